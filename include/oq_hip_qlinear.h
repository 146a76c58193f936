/*
 * oq_hip_qlinear.h -- extension of the C ABI of oq_hip.h: RUNNING the integer core of a `format="qlinear"` file -- QLinearMatMul,
 * com.microsoft::QGemm, MatMulInteger -- on the int8 matrix cores, with exact int32 sums.
 *
 * oq_hip.h (OQ_ABI_VERSION 2), oq_hip_half.h (OQ_HALF_EXTENSION_VERSION 1) and oq_hip_nbits.h (OQ_NBITS_EXTENSION_VERSION 1) stay
 * what they are; the entry points below live in the same library and follow the same conventions (device pointers, asynchronous
 * on `stream`, no allocation, 0 or a negative oq_status, oq_last_error()).  Every refusal happens on the host before the first
 * launch: no output is touched.
 *
 *       acc[m, n] = sum_k (A[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])       int32, exact (two's-complement wrap, like the operator)
 *       Y[m, n]   = epilogue(acc[m, n])
 *
 * Arithmetic.  v_mfma_i32_16x16x64_i8 is signed x signed.  An unsigned operand is flipped to signed while it is staged (x ^ 0x80
 * per byte) and its zero point moves by 128: with a' = a - 128 [A unsigned], za' = a_zp - 128 [A unsigned], and b', zb' likewise,
 *
 *       acc = S - zb'[n] * rowsum_k(a')[m] - za' * colsum_k(b')[n] + K * za' * zb'[n],        S = sum_k a' * b' from the matrix cores.
 *
 * The row and column sums are int32 vectors in the workspace, written by two prologue kernels; a sum is computed unless its
 * multiplier is known to be zero on the host (the other operand is signed and its zero-point pointer is NULL).  The correction
 * runs in uint32: a wrap is defined.  Every parameter is read on the device; nothing synchronises with the host.  Deterministic:
 * integer sums, no atomics; where K is split across workgroups (few output tiles: small M) the partial sums go through int32
 * workspace slabs that one kernel adds, corrects and finishes.
 *
 * Epilogue, every step one fp32 rounding, in this order (the library is built without contraction):
 *   OQ_QL_OUT_I32    Y = acc                                                           (MatMulInteger)
 *   OQ_QL_OUT_F32    Y = t = fp32(acc) * fl(a_scale * b_scale[n])                      (QGemm without y_scale)
 *   OQ_QL_OUT_U8/I8  q = rint(t / y_scale) + y_zp, saturated to the type               (rint: half to even; the division is IEEE)
 *
 * Left out, deliberately (OQ_ERR_UNSUPPORTED, by name -- such nodes stay on the caller's expanded route):
 *   per-row activation parameters, transA, alpha != 1 (`flags`), fp16 scales and outputs, a cache of B's column sums across calls.
 * The QuantizeLinear in front and the DequantizeLinear behind -- the body of a `quant`-domain QLinearMatMul / QLinearGemm function --
 * are fused by the entry points of oq_hip_qlinear_function.h (fp32 in, fp32 out); this header's stay on 8-bit operands.
 */
#ifndef OQ_HIP_QLINEAR_H
#define OQ_HIP_QLINEAR_H

#include "oq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QLINEAR_EXTENSION_VERSION 1

/* element type of A and of B (each has its own) */
typedef enum { OQ_QL_U8 = 0, OQ_QL_I8 = 1 } oq_ql_type;
/* how B lies in memory */
typedef enum { OQ_QL_KN = 0 /* B[k * ldb + n]: QLinearMatMul, QGemm transB = 0 */, OQ_QL_NK = 1 /* B[n * ldb + k]: QGemm transB = 1 */ } oq_ql_layout;
/* what Y holds */
typedef enum { OQ_QL_OUT_I32 = 0, OQ_QL_OUT_F32 = 1, OQ_QL_OUT_U8 = 2, OQ_QL_OUT_I8 = 3 } oq_ql_out;

/* `flags`: properties of the node the kernel has no route for; a set bit is answered with OQ_ERR_UNSUPPORTED by name, so that a
 * caller can hand the node's description over as it is and keep its own route on refusal */
#define OQ_QL_PER_ROW_A 1 /* a_scale / a_zero_point per row of A */
#define OQ_QL_TRANS_A 2   /* QGemm transA */
#define OQ_QL_ALPHA 4     /* QGemm alpha != 1 */

/* OQ_QLINEAR_EXTENSION_VERSION of the loaded library */
int32_t oq_qlinear_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A             [M, K] row-major of `a_type`, leading dimension lda >= K, any byte alignment.  Rows that are not 16-byte aligned
 *                 take narrower loads and give the same bytes.
 *   B             of `b_type`; OQ_QL_KN: [K, N] with ldb >= N; OQ_QL_NK: [N, K] with ldb >= K; any byte alignment (KN rows that
 *                 are not 4-byte aligned take byte loads).
 *   a_scale       one fp32;  a_zero_point  one element of a_type, NULL: 0.
 *   b_scale       one fp32, or [N] when b_per_column != 0;  b_zero_point  one element of b_type or [N] likewise, NULL: 0.
 *   C             NULL, or int32 [N] (QGemm's bias at scale a_scale * b_scale): added to acc before anything else.
 *   y_scale       one fp32;  y_zero_point  one element of Y's type, NULL: 0.  Read for OQ_QL_OUT_U8 / _I8 only.
 *                 a_scale and b_scale are required unless out is OQ_QL_OUT_I32, y_scale for OQ_QL_OUT_U8 / _I8.
 *   Y             [M, N] of int32 / fp32 / uint8 / int8 per `out`, leading dimension ldy >= N, aligned to its element; columns
 *                 N ... ldy - 1 are not written.
 *   bounds        M, K, N, lda, ldb, ldy in 1 ... 2^31 - 1; M * lda, rows(B) * ldb and M * ldy at most 2^40 (oq_hip.h).
 *   workspace     256-byte aligned, oq_qlinear_matmul_workspace_bytes(M, K, N) = R + C + S, a function of the shape alone:
 *                   R  (the row sums of A)     = r256(M * 4),                                  r256: rounded up to 256
 *                   C  (the column sums of B, for a KN matrix as 8 partial sums over eighths of K)  = 8 * r256(N * 4),
 *                   S  (the split-K slabs)     = splits > 1 ? r256(splits * M * N * 4) : 0, with (as in oq_hip_nbits.h)
 *                        BM = M <= 32 ? 32 : 128,  tiles = ceil(M / BM) * ceil(N / 128),  steps = ceil(K / 64),
 *                        want = tiles >= 128 ? 1 : min(8, steps, 256 / tiles),  splits = ceil(steps / ceil(steps / want)).
 *                 The query returns 0 for a request outside the bounds.
 *   checks        null pointers, the type / layout / output codes, unknown flags, alignment and the bounds
 *                 OQ_ERR_INVALID_ARGUMENT; a set bit of `flags` OQ_ERR_UNSUPPORTED; a missing, short or misaligned workspace
 *                 OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qlinear_matmul_workspace_bytes(int64_t M, int64_t K, int64_t N);
int32_t oq_qlinear_matmul(const void* A, int32_t a_type /* oq_ql_type */, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                          const void* a_zero_point, const void* B, int32_t b_type /* oq_ql_type */, int32_t b_layout /* oq_ql_layout */,
                          int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point, int32_t b_per_column,
                          const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags, int32_t out /* oq_ql_out */,
                          void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QLINEAR_H */
