/*
 * oq_hip_nbits_fzp.h -- extension of the C ABI of oq_hip.h: the TILE route of com.microsoft::MatMulNBits for FLOATING-POINT zero
 * points [N, blocks], as HQQ files store them, any M, run from the packed blob this library writes (OQ_LAYOUT_NBITS).
 *
 * oq_hip.h (OQ_ABI_VERSION 2), oq_hip_half.h, oq_hip_nbits.h (OQ_NBITS_EXTENSION_VERSION 1) and oq_hip_nbits_decode.h
 * (OQ_NBITS_DECODE_EXTENSION_VERSION 1) stay what they are: oq_matmul_nbits still refuses OQ_NBITS_FLOAT_ZERO_POINTS by name, and
 * oq_matmul_nbits_decode still takes them for 1 ... 16 rows.  The entry points below live in the same library and follow the same
 * conventions (device pointers, asynchronous on `stream`, no allocation, no host synchronisation, capturable into a hipGraph, 0 or
 * a negative oq_status, oq_last_error()).  Every refusal happens on the host before the first launch: no output is touched.
 *
 *       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
 *
 * Arithmetic.  Every zero point is split once, in fp32:
 *       zi = clamp(rint(zp), 0, 2^bits - 1)  (ties to even)          f = zp - zi
 * q - zi is an integer in [-255, 255], exact in fp16 and in bf16: per k-group the products A_g . (q - zi)_g run on the matrix cores
 * (v_mfma_f32_16x16x32_f16 / _bf16) into an fp32 accumulator acc, exactly as in oq_matmul_nbits, and the same instructions against
 * a fragment of ones give rs, the sums of A's rows over the same k.  The group's sum is then
 *       t = fma(-f, rs, acc)          sum = fma(t, scale, sum)
 * |f| <= 0.5 while zp lies in [0, 2^bits - 1]; a zero point outside that range is legal (HQQ writes them for one-signed groups)
 * and f takes what the clamp cut off.  An integer-valued zero point inside the range has f = 0: the call then gives the bytes of
 * oq_matmul_nbits on the same zero points packed.  The tile, the plan, the fp32-A pieces (two fp16 pieces under one power-of-two
 * scale per row), the split of K through slabs added in slab order, and the one rounding to Y's type after the bias are those of
 * oq_matmul_nbits (oq_hip_nbits.h).  No [N, K] matrix exists at any point.  Deterministic: no atomics.  A NaN in a row of A
 * poisons exactly that row; a NaN zero point poisons exactly its column; a row of A that holds an infinity gives NaN or infinity
 * in that row only.  The error bound and its derivation: DESIGN.md 4.30.
 *
 * Left out (OQ_ERR_UNSUPPORTED, by name): integer zero points, packed uint8 or NULL (oq_matmul_nbits is their route); g_idx; bits
 * other than 4 and 8; a group_size that is no multiple of 32 (group_size 16 stays with oq_matmul_nbits_decode up to 16 rows and
 * with the caller's expanded route beyond).
 */
#ifndef OQ_HIP_NBITS_FZP_H
#define OQ_HIP_NBITS_FZP_H

#include "oq_hip_nbits_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_NBITS_FZP_EXTENSION_VERSION 1

/* OQ_NBITS_FZP_EXTENSION_VERSION of the loaded library */
int32_t oq_nbits_fzp_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A            [M, K] row-major of type `atype`, leading dimension lda >= K (elements), aligned to its element.  Rows that are
 *                not 16-byte aligned are legal, take narrower loads and give the same bytes.
 *   B            the MatMulNBits blob [N, blocks, g * bits / 8], blocks = ceil(K / g), 16-byte aligned; bits 4 (low nibble = even k)
 *                or 8.  K need not be a multiple of g: the padded positions contribute nothing, to acc or to rs, whatever they hold.
 *   group_size   g, any multiple of 32 (32 ... 256, or K of a group_size = -1 file).
 *   scales       [N, blocks]; scales_type OQ_NBITS_F32, or `atype`.  Applied in fp32.  Aligned to their element.
 *   zero_points  [N, blocks] floating point; zero_points_type OQ_NBITS_F32, or `atype`.  Aligned to their element.  NULL and
 *                OQ_NBITS_ZP_PACKED_U8 are refused by name.
 *   bias         NULL, or [N] of type `atype`; added in fp32 before the one rounding.
 *   flags        OQ_NBITS_FLOAT_ZERO_POINTS is accepted (set or not: zero_points_type says what they are); OQ_NBITS_G_IDX is
 *                refused by name.
 *   Y            [M, N] of type `atype`, leading dimension ldy >= N; columns N ... ldy - 1 are not written.
 *   bounds       M, K, N, lda, ldy in 1 ... 2^31 - 1; M * lda, M * ldy and N * blocks * g at most 2^40 (oq_hip.h).
 *   workspace    256-byte aligned, oq_matmul_nbits_fzp_workspace_bytes(M, K, N, group_size, atype) = P + S, exactly those of
 *                oq_matmul_nbits (the row sums live in registers and add nothing):
 *                  P  (fp32 A only: the two fp16 pieces and a scale exponent per row)
 *                       = 2 * r256(M * 8 * ceil(K / 8) * 2) + r256(M * 4),                  r256: rounded up to 256
 *                  S  (the split-K slabs) = splits > 1 ? r256(splits * M * N * 4) : 0, with
 *                       BM = M <= 32 ? 32 : 128,  tiles = ceil(M / BM) * ceil(N / 128),  steps = ceil(K / 64),
 *                       want = tiles >= 128 ? 1 : min(8, steps, 256 / tiles),  splits = ceil(steps / ceil(steps / want)).
 *                May be NULL when that is 0.  The query returns 0 for a request outside the bounds or with an unknown atype.
 *   checks       null pointers, the type codes, alignment and the bounds OQ_ERR_INVALID_ARGUMENT; bits, group_size, g_idx and
 *                integer zero points OQ_ERR_UNSUPPORTED; a missing, short or misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_matmul_nbits_fzp_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype);
int32_t oq_matmul_nbits_fzp(const void* A, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, const void* B, int32_t bits,
                            int64_t N, int64_t group_size, const void* scales, int32_t scales_type /* oq_nbits_type */,
                            const void* zero_points, int32_t zero_points_type /* oq_nbits_type */, const void* bias, int32_t flags, void* Y,
                            int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_NBITS_FZP_H */
