/*
 * oq_hip_qdq_function.h -- extension of the C ABI of oq_hip.h: one CALL of a `quant`-domain QDQ function with QUANTIZED ACTIVATIONS
 * (the default output format, QConfig(weights, input_activations[, output_activations])) in one library call -- fp32 X in, fp32 Y
 * out, the product on the int8 matrix cores.  The function's body is
 *
 *       QuantizeLinear | DynamicQuantizeLinear (X)  ->  DequantizeLinear  ->  MatMul | Gemm on DequantizeLinear(W) (and (B))
 *                                                   [ ->  QuantizeLinear | DynamicQuantizeLinear  ->  DequantizeLinear ]
 *
 * After the input Q -> DQ the activation is exactly (q_x - zp_x) * x_scale with an 8-bit q_x, so the product is exactly
 * x_scale * w_scale[n] * sum_k (q_x - zp_x)(W - zp_w[n]): an integer sum, computed on v_mfma_i32_16x16x64_i8 by the tile GEMM of
 * oq_hip_qlinear.h.  oq_qdq_matmul (oq_hip_qdq.h) accumulates the same products in fp32; the two differ by that rounding (`error`).
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and the other extensions stay what they are; nothing is rerouted.  The entry points below live in the
 * same library and follow the same conventions: device pointers only, asynchronous on `stream`, no allocation, no host
 * synchronisation, capturable into a HIP graph, no atomics, deterministic; 0 or a negative oq_status, oq_last_error().  Every refusal
 * happens on the host before the first launch: no output is touched.  EVERY PARAMETER IS READ ON THE DEVICE.
 *
 * Arithmetic, every step one fp32 rounding (the library is built without contraction; the divisions are IEEE):
 *
 *   dynamic parameters of a tensor T (the bytes of the operator DynamicQuantizeLinear as the package's runner computes it):
 *       lo = min(min T, 0)   hi = max(max T, 0)   scale = (hi - lo) / 255   safe = scale == 0 ? 1 : scale
 *       zp = rint(clamp(-lo / safe, 0, 255))      q(t) = clamp(rint(t / safe) + zp, 0, 255)      dq(q) = (q - zp) * scale
 *       min / max propagate NaN, as every reduction of this library does: a NaN anywhere in T makes scale NaN and every element of
 *       Y NaN (also through a static output Q -> DQ, which passes a NaN v on instead of saturating it).
 *   static input:   q_x = sat(rint(X / x_scale) + fp32(x_zp)), the quantizer of oq_hip_qlinear_function.h as it is (a NaN of X
 *                   gives the bottom of the type)
 *   S[m, n] = sum_k (q_x[m, k] - zp_x) * (W[k, n] - zp_w[n])                       int32, exact
 *   v       = fp32(S) * fl(x_scale * w_scale[n])                                   ; Gemm:  v = v + (fp32(B[n]) - fp32(b_zp)) * b_scale
 *   OQ_QDQ_NONE:     Y = v
 *   OQ_QDQ_STATIC:   q = clamp(rint(v / out_scale) + fp32(out_zp), type range);  Y = (q - fp32(out_zp)) * out_scale
 *   OQ_QDQ_DYNAMIC:  the dynamic parameters of the M x N values v, then Y = dq(q(v))
 *
 *   error        against real arithmetic on the same integers and fp32 parameters, OQ_QDQ_NONE:
 *                |Y - R| <= 4 * 2^-24 * (|R_product| + |bias|): the rounding of fp32(S) (exact below 2^24), of x_scale * w_scale[n]
 *                and of their product, and the one of the bias addition.
 *
 * Launches.  static input: the quantizing prologue (one wave per row: the int8 image of X and its row sums in one pass), the column
 * sums of W (where x_zp' != 0 can be), the tile GEMM, and for a split K the reduce: 2 ... 4.  dynamic input: ahead of those a min / max
 * pass over X (one pair per workgroup into the workspace) and a one-workgroup kernel that forms safe, scale and zp there: + 2.
 * dynamic output: the GEMM's epilogue (the reduce, where K is split) writes v to Y and leaves one (min, max) per workgroup, taken
 * over valid elements only; one finishing launch reduces the pairs, forms the parameters and rewrites Y in place: + 1.
 *
 * Left out, deliberately:
 *   a decode route (M <= 16)      such calls are correct here (the 32-row tile, K split across workgroups) but not tuned.
 *   no input Q -> DQ              is not a mode of this call: those functions keep oq_qdq_matmul.
 *   fp16 / bf16 X, grouped W, 4-bit W      OQ_ERR_UNSUPPORTED, by name.
 *   int32 activation types; a cache of W's column sums across calls.
 */
#ifndef OQ_HIP_QDQ_FUNCTION_H
#define OQ_HIP_QDQ_FUNCTION_H

#include "oq_hip_qdq.h"
#include "oq_hip_qlinear_function.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_FUNCTION_EXTENSION_VERSION 1

/* how an activation is quantized: not at all (the output only), with given parameters, with parameters computed from the tensor */
typedef enum { OQ_QDQ_NONE = 0, OQ_QDQ_STATIC = 1, OQ_QDQ_DYNAMIC = 2 } oq_qdq_mode;

/* OQ_QDQ_FUNCTION_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_function_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   X            [M, K] row-major fp32 (`atype` OQ_NBITS_F32; OQ_NBITS_F16 / _BF16 are refused by name), leading dimension
 *                lda >= K in elements, 4-byte aligned.  Rows that are not 16-byte aligned take narrower loads and give the same
 *                bytes.  No element at or beyond column K is read.
 *   x_mode       OQ_QDQ_STATIC: x_type (OQ_QL_U8 / OQ_QL_I8), x_scale (required), x_zero_point (one element of x_type; NULL: 0).
 *                OQ_QDQ_DYNAMIC: uint8, the parameters are computed from X; x_type, x_scale and x_zero_point are not read.
 *   W            [K, N] row-major, one byte per value, `wtype` OQ_UINT8 or OQ_INT8 (oq_qtype; OQ_UINT4 / OQ_INT4 are refused by name),
 *                leading dimension ldw >= N; any byte alignment of the base and of the rows.
 *   granularity  OQ_TENSOR or OQ_CHANNEL (one w_scale / w_zero_point per column n); OQ_GROUP is refused by name.  w_scale
 *                (required) fp32, w_zero_point of W's type, NULL: 0.
 *   B            NULL (MatMul), or the int32 [N] bias of a Gemm with b_scale (one fp32, required then) and b_zero_point (one
 *                int32, NULL: 0): dequantized in the epilogue.
 *   out_mode     OQ_QDQ_NONE; OQ_QDQ_STATIC: out_type (OQ_QL_U8 / OQ_QL_I8), out_scale (required), out_zero_point (one element of
 *                out_type, NULL: 0); OQ_QDQ_DYNAMIC: uint8, out_type / out_scale / out_zero_point are not read.
 *   Y            [M, N] fp32, leading dimension ldy >= N, 4-byte aligned; columns N ... ldy - 1 are not written.
 *   bounds       those of oq_qlinear_matmul (oq_hip_qlinear.h), and K <= 33025: beyond it 255 * 255 * K passes 2^31 - 1, an int32
 *                sum could wrap, and here -- unlike in the operator QLinearMatMul -- a wrap is an error of the product.
 *   workspace    256-byte aligned.  oq_qdq_function_workspace_bytes(M, K, N, x_mode, out_mode) = Q + R + C + S + P + PX + PO:
 *                Q + R + C + S  of oq_qlinear_function_workspace_bytes(M, K, N);
 *                P  = 256 where x_mode is OQ_QDQ_DYNAMIC (safe, scale, zp), else 0;
 *                PX = r256(8 * min(ceil(M / 4), 2048)) where x_mode is OQ_QDQ_DYNAMIC (the pairs of the pass over X), else 0;
 *                PO = r256(8 * G) where out_mode is OQ_QDQ_DYNAMIC, else 0: G the workgroups that finish v -- the tiles of the
 *                     plan for one split (oq_hip_qlinear.h, `workspace`), ceil(M * N / 256) for a split K.
 *                The query returns 0 (and sets oq_last_error) for a request outside the bounds or with an unknown mode.
 *   checks       null pointers, the type / mode / granularity codes, alignment of X / Y / B / the scales and the bounds
 *                OQ_ERR_INVALID_ARGUMENT; fp16 / bf16 X, OQ_GROUP, 4-bit W and K > 33025 OQ_ERR_UNSUPPORTED; a missing, short or
 *                misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_function_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode /* oq_qdq_mode */, int32_t out_mode /* oq_qdq_mode */);
int32_t oq_qdq_function(const void* X, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, int32_t x_mode /* oq_qdq_mode */,
                        int32_t x_type /* oq_ql_type */, const float* x_scale, const void* x_zero_point, const void* W,
                        int32_t wtype /* oq_qtype */, int64_t N, int64_t ldw, int32_t granularity /* oq_strategy */, int64_t group_size,
                        const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale, const int32_t* b_zero_point,
                        int32_t out_mode /* oq_qdq_mode */, int32_t out_type /* oq_ql_type */, const float* out_scale,
                        const void* out_zero_point, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_FUNCTION_H */
