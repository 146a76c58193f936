/*
 * oq_hip_qlinear_function.h -- extension of the C ABI of oq_hip.h: one CALL of a `quant`-domain function QLinearMatMul / QLinearGemm
 * of a `format="qlinear"` file in one library call -- fp32 X in, fp32 Y out.  The function's body is
 *
 *       QuantizeLinear(X, x_scale, x_zero_point)  ->  QLinearMatMul | com.microsoft::QGemm  ->  DequantizeLinear(out, out_scale, out_zero_point)
 *
 * and the bytes of Y are those of running the three nodes one after the other.  A is quantized on its way into the integer product
 * and Y is dequantized in the epilogue; neither the 8-bit A nor the 8-bit output is handed to the caller.
 *
 * oq_hip_qlinear.h (OQ_QLINEAR_EXTENSION_VERSION 1) and oq_hip_qlinear_decode.h (OQ_QLINEAR_DECODE_EXTENSION_VERSION 1) stay what they
 * are: their entry points, codes, plans, workspace formulas and refusals are unchanged, and nothing is rerouted.  The entry points
 * below live in the same library, follow the same conventions (device pointers, asynchronous on `stream`, no allocation, 0 or a
 * negative oq_status, oq_last_error()) and take the argument list of oq_qlinear_matmul with the differences named under `operands`.
 * Every refusal happens on the host before the first launch: no output is touched.
 *
 * Arithmetic, every step one fp32 rounding (the library is built without contraction; the divisions are IEEE):
 *
 *       q_a[m, k] = sat_a( rint( X[m, k] / a_scale ) + fp32(a_zp) )      rint: half to even; sat_a clamps in fp32 to A's type
 *                                                                       (0 ... 255 or -128 ... 127), then converts
 *       acc[m, n] = sum_k (q_a[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])          int32, exact, as in oq_hip_qlinear.h
 *       q_y       = rint( fp32(acc) * fl(a_scale * b_scale[n]) / y_scale ) + fp32(y_zp), saturated to `y_type`     (OQ_QL_OUT_U8 / _I8)
 *       Y[m, n]   = (fp32(q_y) - fp32(y_zp)) * y_scale
 *
 * The quantizer: +-inf and quotients beyond the type's range saturate.  A NaN gives the BOTTOM of the type (the clamp is
 * fminf(fmaxf(., lo), hi), and fmaxf returns its other operand) -- as the epilogue of oq_hip_qlinear.h already does; the expanded
 * route's cast of a NaN is undefined.  It is not oq_quantize's element function, which converts to int32 ahead of the zero point.
 *
 * Routes.
 *   oq_qlinear_function           any M.  A prologue kernel (one wave per row) quantizes X once into an int8 image in the workspace,
 *                                 leading dimension K rounded up to 16, and writes the row sums of that image in the same pass; the
 *                                 tile GEMM of oq_hip_qlinear.h then runs on the image, with its plan and its split-K reduce, and
 *                                 the dequantizing step at the end of the epilogue.
 *   oq_qlinear_function_decode    M = 1 ... 16.  The kernels, the plan and the slabs of oq_hip_qlinear_decode.h; a workgroup quantizes
 *                                 its slice of X on the way into LDS, where it lies as the same bytes as on the byte route.  At most
 *                                 two launches, no prologue, no atomics, capturable.  The bytes of Y are those of oq_qlinear_function.
 *
 * Left out, deliberately (OQ_ERR_UNSUPPORTED, by name): per-row or dynamic activation parameters, transA, alpha != 1 (`flags`),
 * M >= 17 on the decode entry point; fp16 / bf16 X, scales or Y; a cache of B's column sums across calls.
 */
#ifndef OQ_HIP_QLINEAR_FUNCTION_H
#define OQ_HIP_QLINEAR_FUNCTION_H

#include "oq_hip_qlinear_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QLINEAR_FUNCTION_EXTENSION_VERSION 1

/* OQ_QLINEAR_FUNCTION_EXTENSION_VERSION of the loaded library */
int32_t oq_qlinear_function_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   operands      as for oq_qlinear_matmul (oq_hip_qlinear.h), except:
 *   A             [M, K] row-major fp32 (the function's X), leading dimension lda >= K in elements, 4-byte aligned.  Rows that are
 *                 not 16-byte aligned take narrower loads and give the same bytes.  No element at or beyond column K is read.
 *   a_type        the type A is quantized to; a_scale (required) and a_zero_point (one element of a_type, NULL: 0 -- with
 *                 OQ_QL_U8 the operator's default) are the function's x_scale / x_zero_point.
 *   y_scale       required;  y_zero_point  one element of `y_type`, NULL: 0: the function's out_scale / out_zero_point.
 *   y_type        OQ_QL_U8 or OQ_QL_I8: the type the product is quantized to before it is dequantized (in the place of `out`).
 *   Y             [M, N] fp32, leading dimension ldy >= N, 4-byte aligned; columns N ... ldy - 1 are not written.
 *   workspace     256-byte aligned.
 *                 oq_qlinear_function_workspace_bytes(M, K, N) = Q + R + C + S with Q = r256(M * r16(K)) (the int8 image of A; r16:
 *                 rounded up to 16) ahead of R, C, S of oq_qlinear_matmul_workspace_bytes(M, K, N).
 *                 oq_qlinear_function_decode_workspace_bytes(M, K, N, b_layout) = S of oq_qlinear_matmul_decode_workspace_bytes;
 *                 `workspace` may be NULL when it is 0.
 *                 A query returns 0 (and sets oq_last_error) for a request outside the bounds; the decode query also for M > 16 and
 *                 for an unknown layout.
 *   checks        null pointers, the type / layout codes, unknown flags, alignment of A / Y / C / the scales and the bounds
 *                 OQ_ERR_INVALID_ARGUMENT; a set bit of `flags`, and M >= 17 on the decode entry point, OQ_ERR_UNSUPPORTED; a missing,
 *                 short or misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qlinear_function_workspace_bytes(int64_t M, int64_t K, int64_t N);
int32_t oq_qlinear_function(const float* A, int32_t a_type /* oq_ql_type */, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                            const void* a_zero_point, const void* B, int32_t b_type /* oq_ql_type */, int32_t b_layout /* oq_ql_layout */,
                            int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point, int32_t b_per_column,
                            const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags, int32_t y_type /* oq_ql_type */,
                            float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

size_t oq_qlinear_function_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t b_layout /* oq_ql_layout */);
int32_t oq_qlinear_function_decode(const float* A, int32_t a_type /* oq_ql_type */, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                                   const void* a_zero_point, const void* B, int32_t b_type /* oq_ql_type */, int32_t b_layout /* oq_ql_layout */,
                                   int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point, int32_t b_per_column,
                                   const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags,
                                   int32_t y_type /* oq_ql_type */, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QLINEAR_FUNCTION_H */
