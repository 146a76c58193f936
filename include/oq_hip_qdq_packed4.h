/*
 * oq_hip_qdq_packed4.h -- extension of the C ABI of oq_hip.h: the product of oq_hip_qdq.h run from a 4-bit weight as the file
 * stores it.  The reference's default output format (QFormat.QDQ) writes every 4-bit weight that MatMulNBits does not take -- QInt4
 * symmetric, 4 bits per tensor or per channel, 4-bit Gemm, any 4-bit weight with quantized activations, groups that fail the
 * power-of-two rule -- as an ONNX INT4 / UINT4 initializer: [K, N], two values per byte in flat order, the even index in the low
 * nibble.  It is what OQ_LAYOUT_KN_PACKED4 (oq_hip.h) writes on the quantize side.  oq_qdq_matmul reads such a weight only after it
 * has been unpacked to one value per byte; the entry point below reads the bytes as stored: half the memory, half the weight read.
 *
 * oq_hip.h (OQ_ABI_VERSION 2), oq_hip_qdq.h and the other extensions stay what they are; the entry points below live in the same
 * library and follow the conventions of oq_hip_qdq.h (device pointers, asynchronous on `stream`, no allocation, 0 or a negative
 * oq_status, oq_last_error()).  Every refusal happens on the host before the first launch: no output is touched.
 *
 *       Y[M, N] = A[M, K] . dequant(W) (+ bias)          dequant(W)[k, n] = (q[k, n] - zp[i]) * scale[i]
 *             q[k, n] = nibble (n & 1) of byte W[k * ldw + n / 2]
 *             i = 0 (OQ_TENSOR) | n (OQ_CHANNEL) | n * (K / g) + k / g (OQ_GROUP: groups of g along K)
 *
 * Arithmetic: that of oq_qdq_matmul, operand for operand; q - zp is an integer in [-15, 15].  For the same integers the two entry
 * points give the same bytes.  No atomics; deterministic; capturable into a HIP graph.
 *
 * Left out, deliberately:
 *   an odd N                        the rows of a flat-packed [K, N] then start on alternating nibbles: no byte matrix
 *                                   (OQ_ERR_UNSUPPORTED, by name).  Such a tensor is unpacked and goes to oq_qdq_matmul.
 *   packed zero points              they stay one value per byte: 1 | N | N * K / g values, nothing to gain.
 *   a decode route (M <= 16)        such calls run on the 32-row tile with K split across workgroups, as in oq_qdq_matmul.
 *   group_size % 32 != 0, K % group_size != 0      as in oq_qdq_matmul (OQ_ERR_UNSUPPORTED, by name).
 */
#ifndef OQ_HIP_QDQ_PACKED4_H
#define OQ_HIP_QDQ_PACKED4_H

#include "oq_hip_qdq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_PACKED4_EXTENSION_VERSION 1

/* OQ_QDQ_PACKED4_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_packed4_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A, scales, bias, Y, granularity, group_size, workspace, stream      as in oq_qdq_matmul (oq_hip_qdq.h).
 *   W            [K, N] values as [K, N / 2] bytes, row-major; `wtype` OQ_UINT4 or OQ_INT4 (oq_qtype; INT4: two's-complement nibbles);
 *                N counts VALUES and is even; leading dimension ldw >= N / 2 counts BYTES; any byte alignment of the base and of the
 *                rows (4-byte aligned rows take dword loads and give the same bytes).  No byte outside [K, N / 2] is read.
 *   zero_points  NULL (0), or one value per byte in the container type (uint8 for OQ_UINT4, int8 for OQ_INT4), inside the 4-bit
 *                range, indexed like the scales.
 *   bounds       those of oq_qdq_matmul, with K * ldw at most 2^40.
 *   workspace    oq_qdq_matmul_packed4_workspace_bytes(M, K, N, atype) = oq_qdq_matmul_workspace_bytes(M, K, N, atype).
 *   checks       those of oq_qdq_matmul, with the same status codes; a type code other than OQ_UINT4 / OQ_INT4 and a short ldw
 *                OQ_ERR_INVALID_ARGUMENT; an odd N OQ_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_matmul_packed4_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t atype);
int32_t oq_qdq_matmul_packed4(const void* A, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, const void* W,
                              int32_t wtype /* OQ_UINT4 | OQ_INT4 */, int64_t N, int64_t ldw /* bytes */, int32_t granularity /* oq_strategy */,
                              int64_t group_size, const void* scales, int32_t scales_type /* oq_nbits_type */, const void* zero_points,
                              const void* bias, void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_PACKED4_H */
