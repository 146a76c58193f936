/*
 * oq_hip_nbits.h -- extension of the C ABI of oq_hip.h: RUNNING a com.microsoft::MatMulNBits node from the packed blob this
 * library writes (OQ_LAYOUT_NBITS, oq_pack_matmul_nbits), without ever expanding the weight.
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and oq_hip_half.h (OQ_HALF_EXTENSION_VERSION 1) stay what they are; the entry points below live
 * in the same library and follow the same conventions (device pointers, asynchronous on `stream`, no allocation, 0 or a
 * negative oq_status, oq_last_error()).  Every refusal happens on the host before the first launch: no output is touched.
 *
 *       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
 *
 * Arithmetic.  q - zp is an integer in [-255, 255]: exact in fp16 and in bf16.  Per k-group the products A_g . (q - zp)_g run on
 * the matrix cores (v_mfma_f32_16x16x32_f16 / _bf16) with that exact B operand and accumulate in fp32; the group's sum is then
 * multiplied by the fp32 scale and added to the running fp32 sum (one fused multiply-add per group).  No [N, K] matrix exists at
 * any point, and an fp16 / bf16 A meets the weight without the weight being rounded to two bytes.  An fp32 A is split into two
 * fp16 pieces under one power-of-two scale per row (22 significand bits; elements below 2^-17 of their row's largest keep an
 * absolute error of 2^-39 of that largest); the pieces live in the workspace and both products share the accumulator.  A row of
 * A that holds a NaN gives a NaN row of Y and touches no other row.  The fp32 sum is rounded to Y's type once, after the bias.
 * Deterministic: no atomics; where K is split across workgroups (few output tiles: small M) the partial sums go through
 * workspace slabs that one kernel adds in slab order.
 *
 * Left out, deliberately (OQ_ERR_UNSUPPORTED, by name -- such nodes stay on the caller's expanded route):
 *   float zero points (HQQ files)   q - zp is then no integer and the exact-operand argument is gone; the correct treatment is a
 *                                   correction term (scale * zp) * rowsum_g(A), a kernel variant of its own.
 *   group_size 16                   two groups would share one 32-deep matrix instruction (any g % 32 != 0 is refused).
 *   g_idx                           a permuted group index per k.
 *   bits other than 4 and 8.
 * M = 1 ... 16 are correct here (a 32-row tile, K split across workgroups) but not tuned: the decode route is an entry point of its
 * own, oq_matmul_nbits_decode (oq_hip_nbits_decode.h), which also takes float zero points and group_size 16.
 */
#ifndef OQ_HIP_NBITS_H
#define OQ_HIP_NBITS_H

#include "oq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_NBITS_EXTENSION_VERSION 1

/* element type of A, Y and bias */
typedef enum { OQ_NBITS_F32 = 0, OQ_NBITS_F16 = 1 /* IEEE binary16 */, OQ_NBITS_BF16 = 2 /* bfloat16 */ } oq_nbits_type;

/* `flags`: properties of the node the kernel has no route for; a set bit is answered with OQ_ERR_UNSUPPORTED by name, so that a
 * caller can hand the node's description over as it is and keep its own route on refusal */
#define OQ_NBITS_FLOAT_ZERO_POINTS 1 /* the zero points are floating point (HQQ) */
#define OQ_NBITS_G_IDX 2             /* the node carries g_idx */

/* OQ_NBITS_EXTENSION_VERSION of the loaded library */
int32_t oq_nbits_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A            [M, K] row-major of type `atype`, leading dimension lda >= K (elements), aligned to its element.  Rows that are
 *                not 16-byte aligned (K or lda no multiple of 8 halves / 4 floats, an odd element offset of the base) are legal,
 *                take narrower loads and give the same bytes.
 *   B            the MatMulNBits blob [N, blocks, g * bits / 8], blocks = ceil(K / g), 16-byte aligned; bits 4 (low nibble =
 *                even k) or 8.  K need not be a multiple of g: the blob is padded, A has exactly K columns, and the padded
 *                positions contribute nothing whatever bytes they hold.
 *   group_size   g, any multiple of 32 (32 ... 256, or K of a group_size = -1 file).
 *   scales       [N, blocks]; scales_type OQ_NBITS_F32, or `atype` (the FLOAT16 files of half_weights = "native").  Applied in fp32.
 *   zero_points  NULL: 2^(bits - 1).  Otherwise uint8: bits 8 [N, blocks]; bits 4 packed two per byte, [N, ceil(blocks / 2)], low
 *                nibble first -- the pad nibble of an odd block count is never read as data.
 *   bias         NULL, or [N] of type `atype`; added in fp32 before the one rounding.
 *   Y            [M, N] of type `atype`, leading dimension ldy >= N; columns N ... ldy - 1 are not written.
 *   bounds       M, K, N, lda, ldy in 1 ... 2^31 - 1; M * lda, M * ldy and N * blocks * g at most 2^40 (oq_hip.h).
 *   workspace    256-byte aligned, oq_matmul_nbits_workspace_bytes(M, K, N, group_size, atype) = P + S:
 *                  P  (fp32 A only: the two fp16 pieces and a scale exponent per row)
 *                       = 2 * r256(M * 8 * ceil(K / 8) * 2) + r256(M * 4),                  r256: rounded up to 256
 *                  S  (the split-K slabs) = splits > 1 ? r256(splits * M * N * 4) : 0, with
 *                       BM = M <= 32 ? 32 : 128,  tiles = ceil(M / BM) * ceil(N / 128),  steps = ceil(K / 64),
 *                       want = tiles >= 128 ? 1 : min(8, steps, 256 / tiles),  splits = ceil(steps / ceil(steps / want)).
 *                May be NULL when that is 0.  The query returns 0 for a request outside the bounds or with an unknown atype.
 *   checks       null pointers, the type codes, alignment and the bounds OQ_ERR_INVALID_ARGUMENT; bits, group_size and `flags`
 *                OQ_ERR_UNSUPPORTED; a missing, short or misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_matmul_nbits_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype);
int32_t oq_matmul_nbits(const void* A, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, const void* B,
                        int32_t bits, int64_t N, int64_t group_size, const void* scales, int32_t scales_type /* oq_nbits_type */,
                        const uint8_t* zero_points, const void* bias, int32_t flags, void* Y, int64_t ldy, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_NBITS_H */
