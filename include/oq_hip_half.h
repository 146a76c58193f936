/*
 * oq_hip_half.h -- half-precision extension of the C ABI of oq_hip.h: RTN on fp16 / bf16 weights read as they are.
 *
 * oq_hip.h stays what it is (OQ_ABI_VERSION 2); the entry points below live in the same library and follow the same
 * conventions (device pointers, asynchronous on `stream`, no allocation, 0 or a negative oq_status, oq_last_error()).
 * Both conversions to fp32 are exact, so every result is DEFINED as that of the fp32 entry point on the upcast matrix:
 * integers, zero points and fp32 scales match it bit for bit.
 */
#ifndef OQ_HIP_HALF_H
#define OQ_HIP_HALF_H

#include "oq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_HALF_EXTENSION_VERSION 1

/* element type of a 2-byte weight matrix */
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

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_HALF_H */
