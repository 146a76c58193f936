/*
 * oq_hip_qlinear_decode.h -- extension of the C ABI of oq_hip.h: the DECODE route of QLinearMatMul / com.microsoft::QGemm /
 * MatMulInteger, M = 1 ... 16 rows of A against an 8-bit B that is streamed once.
 *
 * oq_hip_qlinear.h (OQ_QLINEAR_EXTENSION_VERSION 1) stays what it is: oq_qlinear_matmul, its plan, its workspace formula and its
 * refusals are unchanged, and nothing is rerouted.  The entry point below lives in the same library, follows the same conventions
 * (device pointers, asynchronous on `stream`, no allocation, 0 or a negative oq_status, oq_last_error()) and takes exactly the
 * argument list, the type / layout / output codes and the `flags` of oq_qlinear_matmul.  Every refusal happens on the host before
 * the first launch: no output is touched.
 *
 *       acc[m, n] = sum_k (A[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])       int32, exact (two's-complement wrap, like the operator)
 *       Y[m, n]   = epilogue(acc[m, n])                                          the epilogue of oq_hip_qlinear.h, the same code
 *
 * So the bytes of Y are those of oq_qlinear_matmul on the same operands, for every output code.
 *
 * Arithmetic.  The products are signed dot4 instructions (four bytes of A against four bytes of B); for M = 5 ... 16 against an
 * OQ_QL_NK matrix whose rows are 16-byte aligned, with K a multiple of 16, they are v_mfma_i32_16x16x64_i8 on registers loaded in the
 * instruction's own operand image (other operands of those tiers keep dot4: the same bytes).  An unsigned operand is flipped
 * to signed on its way into them (x ^ 0x80 per byte) and its zero point moves by 128: with a' = a - 128 [A unsigned],
 * za' = a_zp - 128 [A unsigned], and b', zb' likewise, a slice s of K contributes
 *
 *       S_s - zb'[n] * rowsum_s(a')[m] - za' * colsum_s(b')[n] + K_s * za' * zb'[n]          in uint32: a wrap is defined,
 *
 * K_s the slice's share of K.  B goes from global memory straight into registers, never through LDS, and every byte of it is read
 * once per call: the column sums are taken from the registers that feed the products (one more dot4 -- or MFMA -- against ones per dword),
 * the row sums of A from its slice while it lies staged in LDS.  There is no prologue kernel.  A sum is taken unless its multiplier
 * is known to be zero on the host (the other operand is signed and its zero-point pointer is NULL).  Padded positions -- rows >= M,
 * k >= K, columns >= N -- contribute nothing, whatever lies in memory beyond the extents.
 *
 * Plan (csrc/qlinear_decode_plan.hpp), a function of (M, K, N, b_layout) alone; workgroups of 256 threads:
 *   tier            1 / 4 / 8 / 16 accumulator rows for M = 1 / 2-4 / 5-8 / 9-16
 *   OQ_QL_NK        slice = 1024 k (a lane owns 16 bytes of a row of B, a wave spans the slice), splits = ceil(K / 1024),
 *                   cols_per_block = 16 * ceil(ceil(N / max(1, 512 / splits)) / 16)        (rows of B of one workgroup)
 *   OQ_QL_KN        cols_per_block = 256 (a lane owns 4 columns), want = ceil(W / ceil(N / 256)) with W = 512 (tiers 1, 4) or 256
 *                   (tiers 8, 16), slice = min(1024, 64 * ceil(ceil(K / want) / 64)), splits = ceil(K / slice)
 *   grid            ceil(N / cols_per_block) * splits workgroups: one to two per compute unit of an MI355X on model widths
 * One slice finishes in the first launch.  With more, each slice writes its corrected partial value into an int32 slab and a second
 * launch adds the slabs in slab order, adds C and runs the epilogue.  No atomics, no workgroup waits on another, nothing
 * synchronises with the host: the route can be captured into a graph.  Deterministic.
 *
 * Left out, deliberately (OQ_ERR_UNSUPPORTED, by name): M >= 17 (oq_qlinear_matmul is the route), per-row activation parameters,
 * transA, alpha != 1 (`flags`); as in oq_hip_qlinear.h: fp16 scales and outputs.  A cache of B's column sums across calls is not
 * needed: the sums cost no read.  The QuantizeLinear in front and the DequantizeLinear behind are fused by
 * oq_qlinear_function_decode (oq_hip_qlinear_function.h: fp32 in, fp32 out, this route's kernels and plan).
 */
#ifndef OQ_HIP_QLINEAR_DECODE_H
#define OQ_HIP_QLINEAR_DECODE_H

#include "oq_hip_qlinear.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QLINEAR_DECODE_EXTENSION_VERSION 1

/* OQ_QLINEAR_DECODE_EXTENSION_VERSION of the loaded library */
int32_t oq_qlinear_decode_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   operands      as for oq_qlinear_matmul (oq_hip_qlinear.h), with M = 1 ... 16.  A and B may have any byte alignment: rows of A or
 *                 of an NK matrix that are not 16-byte aligned, and rows of a KN matrix that are not 4-byte aligned, take narrower
 *                 loads and give the same bytes.
 *   workspace     256-byte aligned, oq_qlinear_matmul_decode_workspace_bytes(M, K, N, b_layout) =
 *                   S = splits > 1 ? r256(splits * M * N * 4) : 0                          r256: rounded up to 256
 *                 with `splits` of the plan above.  `workspace` may be NULL when S is 0.  The query returns 0 (and sets
 *                 oq_last_error) for a request outside the bounds, for M > 16 and for an unknown layout.
 *   checks        null pointers, the type / layout / output codes, unknown flags, alignment of Y / C / the scales and the bounds
 *                 OQ_ERR_INVALID_ARGUMENT; M >= 17 and a set bit of `flags` OQ_ERR_UNSUPPORTED; a missing, short or misaligned
 *                 workspace when S > 0 OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qlinear_matmul_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t b_layout /* oq_ql_layout */);
int32_t oq_qlinear_matmul_decode(const void* A, int32_t a_type /* oq_ql_type */, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                                 const void* a_zero_point, const void* B, int32_t b_type /* oq_ql_type */, int32_t b_layout /* oq_ql_layout */,
                                 int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point, int32_t b_per_column,
                                 const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags, int32_t out /* oq_ql_out */,
                                 void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QLINEAR_DECODE_H */
