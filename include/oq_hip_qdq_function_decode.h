/*
 * oq_hip_qdq_function_decode.h -- extension of the C ABI of oq_hip.h: the decode route of oq_hip_qdq_function.h.  The same call -- one
 * `quant`-domain QDQ function with QUANTIZED ACTIVATIONS, fp32 X in, fp32 Y out, an 8-bit weight as the [K, N] bytes the file stores
 * -- for 1 ... 16 rows of X, where the weight is all the traffic there is: W is read ONCE, straight from global memory into the
 * registers that feed v_mfma_i32_16x16x64_i8, with no tile to pad to, no pass for its column sums and no image of X in memory.
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and the other extensions stay what they are; nothing is rerouted: oq_qdq_function takes every M, this
 * entry point only M <= 16.  Conventions: those of oq_hip_qdq_function.h -- device pointers only, asynchronous on `stream`, no
 * allocation, no host synchronisation, capturable into a HIP graph, no atomics, deterministic; 0 or a negative oq_status,
 * oq_last_error().  Every refusal happens on the host before the first launch: no output is touched.  EVERY PARAMETER IS READ ON THE
 * DEVICE.
 *
 * Arithmetic, every step one fp32 rounding (the library is built without contraction; the divisions are IEEE) -- the block of
 * oq_hip_qdq_function.h:
 *
 *   dynamic parameters of a tensor T:
 *       lo = min(min T, 0)   hi = max(max T, 0)   scale = (hi - lo) / 255   safe = scale == 0 ? 1 : scale
 *       zp = rint(clamp(-lo / safe, 0, 255))      q(t) = clamp(rint(t / safe) + zp, 0, 255)      dq(q) = (q - zp) * scale
 *       min / max propagate NaN: a NaN anywhere in T makes scale NaN and every element of Y NaN.
 *   static input:   q_x = sat(rint(X / x_scale) + fp32(x_zp)) (a NaN of X gives the bottom of the type)
 *   S[m, n] = sum_k (q_x[m, k] - zp_x) * (W[k, n] - zp_w[n])                       int32, exact
 *   v       = fp32(S) * fl(x_scale * w_scale[n])                                   ; Gemm:  v = v + (fp32(B[n]) - fp32(b_zp)) * b_scale
 *   OQ_QDQ_NONE:     Y = v
 *   OQ_QDQ_STATIC:   q = clamp(rint(v / out_scale) + fp32(out_zp), type range);  Y = (q - fp32(out_zp)) * out_scale
 *   OQ_QDQ_DYNAMIC:  the dynamic parameters of the M x N values v, then Y = dq(q(v))
 *
 * The result is THE SAME BYTES as oq_qdq_function for every accepted call: both form the exact S (uint32 arithmetic: any order of
 * the partial sums gives the same bits) and run the same epilogue text on it.
 *
 * What runs (csrc/qdq_function_decode.hip):
 *   product      one kernel for every M <= 16.  A workgroup takes 128 columns and one slice of K; it quantizes its slice of X into LDS
 *                (the static quantizer, or the parameters the launches in front left on the device), and each of its four waves
 *                multiplies a quarter of the slice.  In a wave the 16-lane group g = lane >> 4 walks the rows 64 s + 16 g ... + 15 of
 *                a 64-k span and lane & 15 loads 8 bytes -- 8 columns -- of each, so a group lies on one 128-byte line of a row.  An
 *                unsigned operand is made signed by ^ 0x80 (its zero point moves by 128); after eight 4 x 4 byte transposes the lane
 *                holds, for each of its 8 columns, the 16 consecutive k that are exactly its share of the matrix instruction's B
 *                operand.  No LDS and no cross-lane traffic for W.  With a' and b' the flipped operands and za', zb' their zero points,
 *                    S = sum a' b' - zb'[n] rowsum(a')[m] - za' colsum(b')[n] + K_s za' zb'[n]
 *                per wave, in registers: the column sums come from one more matrix instruction per B operand against a fragment of
 *                ones, the row sums from one per span of the A fragment against ones.  Each is compiled out where its multiplier is
 *                zero whatever the device holds (an int8 X / W with a NULL zero point).
 *   launches     static input:  product [, reduce of the K slices] [, finish of a dynamic output]: static / none is at most two.
 *                dynamic input: min / max of X, its parameters, then the same: three to five.
 *                splits == 1 (one slice of K): the product launch finishes Y itself.
 *   plan         slice  = min(2048, ceil(ceil(K / want) / 64) * 64), want = ceil((M <= 4 ? 512 : 256) / ceil(N / 128))
 *                splits = ceil(K / slice)
 *
 * Left out, deliberately: what oq_hip_qdq_function.h leaves out (grouped W, 4-bit W, fp16 / bf16 X, K > 33025), and
 *   M > 16                        OQ_ERR_UNSUPPORTED, by name: oq_qdq_function is the entry point for such a call.
 */
#ifndef OQ_HIP_QDQ_FUNCTION_DECODE_H
#define OQ_HIP_QDQ_FUNCTION_DECODE_H

#include "oq_hip_qdq_function.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_FUNCTION_DECODE_EXTENSION_VERSION 1

/* OQ_QDQ_FUNCTION_DECODE_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_function_decode_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   every argument as in oq_qdq_function (oq_hip_qdq_function.h), with 1 <= M <= 16.  K <= 33025; ldw >= N; any byte alignment of
 *   W's base and rows (8-byte aligned rows take 8-byte loads and give the same bytes).  No byte outside [K, N] of W and no float of
 *   X at or beyond column K is read; columns N ... ldy - 1 of Y are not written.
 *   workspace    256-byte aligned.  oq_qdq_function_decode_workspace_bytes(M, K, N, x_mode, out_mode) is the sum, each piece rounded
 *                up to 256 bytes, of
 *                  S   splits > 1: splits * M * N * 4, the int32 slabs of the K slices                     (plan: above)
 *                  P   a dynamic input: 12, its parameters (safe, scale, zp)
 *                  PX  a dynamic input: ceil(M / 4) * 8, the (min, max) pairs of the pass over X
 *                  PO  a dynamic output: 8 for every workgroup that finishes Y: ceil(N / 128) of them for splits == 1, else
 *                      ceil(M * N / 256)
 *                `workspace` may be NULL where the sum is 0.  The query returns 0 (and sets oq_last_error) for a request outside
 *                the bounds, with an unknown mode or with M > 16.
 *   checks       those of oq_qdq_function, in its order and with its status codes; M > 16 OQ_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_function_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode /* oq_qdq_mode */, int32_t out_mode /* oq_qdq_mode */);
int32_t oq_qdq_function_decode(const void* X, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, int32_t x_mode /* oq_qdq_mode */,
                               int32_t x_type /* oq_ql_type */, const float* x_scale, const void* x_zero_point, const void* W,
                               int32_t wtype /* oq_qtype */, int64_t N, int64_t ldw, int32_t granularity /* oq_strategy */, int64_t group_size,
                               const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale,
                               const int32_t* b_zero_point, int32_t out_mode /* oq_qdq_mode */, int32_t out_type /* oq_ql_type */,
                               const float* out_scale, const void* out_zero_point, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_FUNCTION_DECODE_H */
