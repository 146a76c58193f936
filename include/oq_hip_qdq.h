/*
 * oq_hip_qdq.h -- extension of the C ABI of oq_hip.h: RUNNING the product of a `quant`-domain QDQ function from the integers the
 * file stores, without ever expanding the weight.  The functions are the reference's default output format (QFormat.QDQ;
 * qfunctions/_qdq/qmatmul.py, qfunctions/_qdq/qgemm.py): QMatMulWeightsOnlyQDQ and its six activation variants, their seven QGemm
 * twins, QMatMulWeightsOnlyGrouped / QGemmWeightsOnlyGrouped.  Each of them dequantizes the whole [K, N] weight to fp32 and then
 * multiplies; the entry point below computes that product from W, its scales and its zero points as they are stored.
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and the other extensions stay what they are; the entry points below live in the same library and
 * follow the conventions of oq_hip_nbits.h (device pointers, asynchronous on `stream`, no allocation, 0 or a negative oq_status,
 * oq_last_error()).  Every refusal happens on the host before the first launch: no output is touched.  The element-type codes
 * are the existing ones: oq_nbits_type (oq_hip_nbits.h) for A, Y, bias and the scales, oq_qtype (oq_hip.h) for W, oq_strategy
 * (oq_hip.h) for the granularity of its parameters.
 *
 *       Y[M, N] = A[M, K] . dequant(W) (+ bias)          dequant(W)[k, n] = (q[k, n] - zp[i]) * scale[i]
 *             i = 0 (OQ_TENSOR) | n (OQ_CHANNEL) | n * (K / g) + k / g (OQ_GROUP: groups of g along K)
 *
 * Arithmetic: that of oq_matmul_nbits, whose error analysis carries over.  q - zp is an integer in [-255, 255], exact in fp16 and
 * in bf16.  Per group the products A_g . (q - zp)_g run on the matrix cores (v_mfma_f32_16x16x32_f16 / _bf16) into an fp32
 * accumulator; the group's sum is folded into the running fp32 sum with the group's fp32 scale by one fused multiply-add.  Per
 * tensor and per column the group is the whole of K.  An fp32 A goes as two fp16 pieces under one power-of-two scale per row.
 * The bias is added in fp32 and the sum rounded to Y's type once.  Few output tiles (small M) split K across workgroups through
 * workspace slabs that one kernel adds in slab order.  No atomics; deterministic; capturable into a HIP graph.  A row of A that
 * holds a NaN gives a NaN row of Y and touches no other row.
 *
 * Left out, deliberately:
 *   a decode route (M <= 16)        such calls are correct here (a 32-row tile, K split across workgroups) but not tuned.
 *   the int8 matrix cores           the static-input variants quantize A to 8 bits first; their product could run as
 *                                   oq_qlinear_matmul with an fp32 output.  That changes the arithmetic class (exact int32 sums
 *                                   instead of fp32 accumulation of dequantized activations) and is the natural follow-up.
 *   packed nibbles                  INT4 / UINT4 tensors arrive here unpacked, one value per byte.
 *   group_size % 32 != 0            two groups would share one 32-deep matrix instruction (OQ_ERR_UNSUPPORTED, by name).
 *   K % group_size != 0             a [K, N] matrix has no padded group (OQ_ERR_UNSUPPORTED, by name).
 */
#ifndef OQ_HIP_QDQ_H
#define OQ_HIP_QDQ_H

#include "oq_hip_nbits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_EXTENSION_VERSION 1

/* OQ_QDQ_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A            [M, K] row-major of type `atype` (oq_nbits_type), leading dimension lda >= K (elements), aligned to its element.
 *                Rows that are not 16-byte aligned are legal, take narrower loads and give the same bytes.
 *   W            [K, N] row-major, one byte per value, `wtype` OQ_UINT8 or OQ_INT8 (oq_qtype), leading dimension ldw >= N; any
 *                byte alignment of the base and of the rows.
 *   granularity  OQ_TENSOR, OQ_CHANNEL (one parameter per column n) or OQ_GROUP (oq_strategy); group_size g is read for
 *                OQ_GROUP only: a multiple of 32 that divides K.
 *   scales       1 | [N] | [N, K / g] values (the flat order of the grouped functions' blocked DequantizeLinear); scales_type
 *                OQ_NBITS_F32, or `atype`.  Applied in fp32.
 *   zero_points  NULL (0), or of W's type, indexed like the scales.
 *   bias         NULL, or [N] of type `atype`; added in fp32 before the one rounding.
 *   Y            [M, N] of type `atype`, leading dimension ldy >= N; columns N ... ldy - 1 are not written.
 *   bounds       M, K, N, lda, ldw, ldy in 1 ... 2^31 - 1; M * lda, M * ldy, K * ldw and N * K at most 2^40 (oq_hip.h).
 *   workspace    256-byte aligned, oq_qdq_matmul_workspace_bytes(M, K, N, atype) = P + S, the P and S of oq_matmul_nbits
 *                (oq_hip_nbits.h, `workspace`): the fp16 pieces and row exponents of an fp32 A, and the split-K slabs.  May be
 *                NULL when that is 0.  The query returns 0 for a request outside the bounds or with an unknown atype.
 *   checks       null pointers, the type and granularity codes, alignment and the bounds OQ_ERR_INVALID_ARGUMENT; group_size
 *                and K % group_size OQ_ERR_UNSUPPORTED; a missing, short or misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_matmul_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t atype);
int32_t oq_qdq_matmul(const void* A, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, const void* W,
                      int32_t wtype /* oq_qtype */, int64_t N, int64_t ldw, int32_t granularity /* oq_strategy */, int64_t group_size,
                      const void* scales, int32_t scales_type /* oq_nbits_type */, const void* zero_points, const void* bias, void* Y,
                      int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_H */
