/*
 * oq_hip_half.h -- half-precision extension of the C ABI of oq_hip.h: RTN on fp16 / bf16 weights and the GPTQ Hessian of
 * fp16 / bf16 activations, both read as they are.
 *
 * oq_hip.h stays what it is (OQ_ABI_VERSION 2); the entry points below live in the same library and follow the same
 * conventions (device pointers, asynchronous on `stream`, no allocation, 0 or a negative oq_status, oq_last_error()).
 * Both conversions to fp32 are exact, so every result is DEFINED as that of the fp32 entry point on the upcast matrix:
 * the integers, zero points and fp32 scales of RTN match it bit for bit; the Hessian (a sum, whose order is the kernel's own)
 * is held to the same tolerance against float64 as the fp32 entry point.
 */
#ifndef OQ_HIP_HALF_H
#define OQ_HIP_HALF_H

#include "oq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_HALF_EXTENSION_VERSION 1

/* element type of a 2-byte matrix (weights, activations) */
typedef enum { OQ_W_F16 = 0 /* IEEE binary16 */, OQ_W_BF16 = 1 /* bfloat16 */ } oq_wtype;

/* OQ_HALF_EXTENSION_VERSION of the loaded library */
int32_t oq_half_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 * A1  core/_algorithms/rtn.py:54-109  _rtn_quantize on W.astype(np.float32), without the fp32 copy: replaces the cast
 *     followed by oq_rtn_quantize_f32 (mse == 0).
 *
 *   W          [K, N], 2 bytes per element of type `wtype`, leading dimension ldw >= N (elements).  Rows that are not
 *              16-byte aligned (odd N, odd ldw, an unaligned base) take narrower loads and give the same bytes.
 *   group_size GROUP only: > 0 (clamped to K), or -1 (= K); K % group_size must be 0 (groups that straddle columns:
 *              OQ_ERR_UNSUPPORTED -- cast and call oq_rtn_quantize_f32).
 *   q_out      OQ_LAYOUT_KN: K*N bytes.  OQ_LAYOUT_NBITS: N*(K/g)*(g*bits/8) bytes (group strategy, g % 16 == 0,
 *              16-byte aligned).  OQ_LAYOUT_KN_PACKED4: OQ_ERR_UNSUPPORTED -- quantize to OQ_LAYOUT_KN and pack with
 *              oq_pack_nibbles.  NULL: parameters only (what oq_rtn_qparams_f32 does for fp32).
 *   scale_out  fp32, zp_out 1 byte each: exactly the arrays of oq_rtn_quantize_f32 (group: entry n*(K/g)+kg).
 *   workspace  oq_rtn_half_workspace_bytes: 0 for groups of up to 256 rows (one fused launch, W read once); channel,
 *              tensor and taller groups run a range pass and a quantize pass over W and keep the partial ranges there
 *              (4-byte aligned).  The query returns 0 for a request outside the bounds of oq_hip.h as well.
 * ------------------------------------------------------------------------------------------- */
size_t oq_rtn_half_workspace_bytes(int64_t K, int64_t N, int32_t strategy, int64_t group_size);
int32_t oq_rtn_quantize_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype,
                            int32_t strategy, int64_t group_size, int32_t symmetric, int32_t reduce_range,
                            float clip_ratio, void* q_out /* NULL: parameters only */, float* scale_out,
                            void* zp_out, int32_t layout, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * G1  core/_algorithms/gptq.py:246-260  _accumulate_hessian on inp.astype(np.float32) (:257), without the fp32 copy:
 *     replaces the cast followed by oq_hessian_accumulate_f32.
 *
 *       H <- H * n_seen / (n_seen + n_add) + 2 / (n_seen + n_add) * X^T X        on the exact fp32 values of X
 *
 *   X          [T, K], 2 bytes per element of type `xtype` (an oq_wtype), leading dimension ldx >= K (elements).  Rows that
 *              are only 2-byte aligned (odd ldx, an unaligned base) take narrower loads and give the same result.
 *   H          fp32 [K, K], contiguous; comes out full and exactly symmetric.  n_add: the sample count (gptq.py:247), not T.
 *   method     there is none: an fp16 x fp16 or bf16 x bf16 product is exact in fp32, so every pair of elements meets in
 *              ONE matrix-core product (v_mfma_f32_16x16x32_f16 / _bf16, fp32 accumulation) with no split, no scale and no
 *              product rounding; only the order of the fp32 sums differs from float64.  At least as exact as every method
 *              of oq_hessian_accumulate_f32.
 *   route      one route for every T >= 1, K >= 1 (K <= 2^17, T * ldx <= 2^40 as in oq_hip.h): a re-layout kernel packs
 *              eight rows of a column into 16 bytes (2 B read, 2 B written per element, zero padding to 32 rows and 256
 *              columns; X is never expanded to fp32 in memory), then 256 x 256 tiles of the upper triangle.  From 993 rows
 *              (two slices of >= 512 rows after padding to 32) T is cut into up to 16 slices where that fills the 256
 *              CUs better, the slices are summed in slice order (deterministic) -- slab permitting: the query budgets 16
 *              slabs of K x K floats for K <= 8192 and 4 above, a smaller workspace gets fewer slices.
 *   workspace  oq_hessian_half_workspace_bytes(T, K): the packed operand and the slabs.  At least the packed operand
 *              (T padded to 32 x K padded to 256 x 2 bytes, + 256) must be given: OQ_ERR_WORKSPACE otherwise, H untouched.
 *              The query returns 0 for a request outside the bounds.
 * ------------------------------------------------------------------------------------------- */
size_t oq_hessian_half_workspace_bytes(int64_t T, int64_t K);
int32_t oq_hessian_accumulate_h16(const void* X, int32_t xtype /* oq_wtype */, int64_t T, int64_t K, int64_t ldx, int64_t n_seen,
                                  int64_t n_add, float* H, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_HALF_H */
