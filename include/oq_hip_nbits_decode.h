/*
 * oq_hip_nbits_decode.h -- extension of the C ABI of oq_hip.h: the DECODE route of com.microsoft::MatMulNBits, M = 1 ... 16 rows
 * of A against the packed blob this library writes (OQ_LAYOUT_NBITS), streamed once from global memory into registers.
 *
 * oq_hip.h (OQ_ABI_VERSION 2), oq_hip_half.h and oq_hip_nbits.h (OQ_NBITS_EXTENSION_VERSION 1) stay what they are: oq_matmul_nbits,
 * its plan, its workspace and its refusals do not change.  The entry points below live in the same library and follow the same
 * conventions (device pointers, asynchronous on `stream`, no allocation, no host synchronisation, capturable into a hipGraph, 0 or
 * a negative oq_status, oq_last_error()).  Every refusal happens on the host before the first launch: no output is touched.
 *
 *       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
 *
 * What the route takes that the tile kernel refuses: floating-point zero points (HQQ files) and group_size 16.
 *
 * Arithmetic.  The blob goes from global memory straight into registers in 16-byte loads -- a lane owns 32 (4 bits) or 16 (8 bits)
 * consecutive k of one row of B -- and is dequantized there; it never passes through LDS.  A's slice is staged once per workgroup.
 *   M <= 4, and every M where a group is no whole number of wave spans (group_size % (512 / bits) != 0: 16, 32, 48, 64, 96 ...):
 *     fp32 on the vector ALU.  A is converted to fp32 exactly (fp16, bf16) or taken as it is (fp32).  In units of 16 k, each inside
 *     one group, d = float(q) - zp (exact for integer zero points; one rounding for fractional ones), acc = fma(a, d, acc) 16 in a
 *     chain, then sum = fma(acc, scale, sum).  The lanes of a row are added in a fixed butterfly.
 *   M >= 5 and group_size % (512 / bits) == 0 (128, 256 ... at 4 bits; 64, 128 ... at 8 bits): v_mfma_f32_16x16x32_f16 / _bf16 with
 *     the rows of A as one operand.  q - zp is an exact fp16 / bf16 operand for integer zero points; for floating ones the operand
 *     is q and a wave span's sum is corrected by zp * rowsum(A), the row sums taken by the same instructions against ones.  An
 *     fp32 A enters as three bf16 pieces, a = b1 + b2 + b3 exactly (no row scale: bf16 has fp32's range).  Per span of 128 / 64 k
 *     the fp32 accumulator is folded with the group's scale, sum = fma(acc - zp * rowsum, scale, sum).
 * Then the K slices are added in slab order, then the bias, then ONE rounding to Y's type.  Deterministic: no atomics, no workgroup
 * waits on another.  A NaN in a row of A poisons exactly that row.  The error bound and its derivation: DESIGN.md 4.26.
 *
 * Plan (csrc/decode_plan.hpp, restated):
 *       tier            = M = 1 ? 1 : M <= 4 ? 4 : M <= 8 ? 8 : 16          accumulator rows of the instantiation
 *       splits          = ceil(K / 1024)                                     one workgroup takes 1024 k; its slice of A sits in LDS
 *       want            = max(1, W / splits)                                 W = 512 workgroups wanted, two per compute unit; W = 256
 *                                                                            for an fp32 A in the tiers 8 and 16 (one fits)
 *       rows_per_block  = 64 * ceil(ceil(N / want) / 64)                     rows of B (columns of Y) of one workgroup
 *       row_blocks      = ceil(N / rows_per_block)
 *       grid            = row_blocks * splits workgroups of 256 threads
 *     splits > 1: every workgroup writes its partial sums to slab `split` of the workspace and a second launch adds the slabs in
 *     slab order (bias and rounding there); splits = 1: the first launch finishes.
 *
 * Left out (OQ_ERR_UNSUPPORTED, by name): M >= 17 (oq_matmul_nbits is the route), g_idx, bits other than 4 and 8, a group_size that
 * is no multiple of 16.
 */
#ifndef OQ_HIP_NBITS_DECODE_H
#define OQ_HIP_NBITS_DECODE_H

#include "oq_hip_nbits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_NBITS_DECODE_EXTENSION_VERSION 1

/* zero_points_type: an oq_nbits_type (OQ_NBITS_F32, or `atype`) for floating-point zero points [N, blocks], or this for uint8 ones
 * packed as oq_matmul_nbits takes them */
#define OQ_NBITS_ZP_PACKED_U8 3

/* OQ_NBITS_DECODE_EXTENSION_VERSION of the loaded library */
int32_t oq_nbits_decode_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   A            [M, K] row-major of type `atype`, M = 1 ... 16, leading dimension lda >= K (elements), aligned to its element.
 *                Rows that are not 16-byte aligned are legal, take narrower loads and give the same bytes.
 *   B            the MatMulNBits blob [N, blocks, g * bits / 8], blocks = ceil(K / g), 16-byte aligned; bits 4 (low nibble = even k)
 *                or 8.  K need not be a multiple of g: the padded positions contribute nothing whatever bytes they hold.
 *   group_size   g, any multiple of 16 from 16 up (K of a group_size = -1 file included, where that is one).
 *   scales       [N, blocks]; scales_type OQ_NBITS_F32, or `atype`.  Applied in fp32.
 *   zero_points  NULL: 2^(bits - 1).  zero_points_type OQ_NBITS_ZP_PACKED_U8: uint8, bits 8 [N, blocks]; bits 4 two per byte,
 *                [N, ceil(blocks / 2)], low nibble first -- the pad nibble of an odd block count is never read as data.
 *                zero_points_type OQ_NBITS_F32 or `atype`: floating point [N, blocks], as HQQ files store them.
 *   bias         NULL, or [N] of type `atype`; added in fp32 before the one rounding.
 *   flags        OQ_NBITS_G_IDX is refused by name; OQ_NBITS_FLOAT_ZERO_POINTS is accepted with a floating zero_points_type.
 *   Y            [M, N] of type `atype`, leading dimension ldy >= N; columns N ... ldy - 1 are not written.
 *   bounds       K, N, lda, ldy in 1 ... 2^31 - 1; M * lda, M * ldy and N * blocks * g at most 2^40 (oq_hip.h).
 *   workspace    256-byte aligned, oq_matmul_nbits_decode_workspace_bytes(M, K, N, group_size, atype) =
 *                  S = splits > 1 ? r256(splits * M * N * 4) : 0,   splits = ceil(K / 1024),   r256: rounded up to 256.
 *                May be NULL when that is 0 (K <= 1024).  The query returns 0 for a request outside the bounds, for M > 16, for a
 *                group_size that is no positive multiple of 16 and for an unknown atype.
 *   checks       null pointers, the type codes, alignment and the bounds OQ_ERR_INVALID_ARGUMENT; M >= 17, bits, group_size and
 *                g_idx OQ_ERR_UNSUPPORTED; a missing, short or misaligned workspace OQ_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t oq_matmul_nbits_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype);
int32_t oq_matmul_nbits_decode(const void* A, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, const void* B,
                               int32_t bits, int64_t N, int64_t group_size, const void* scales, int32_t scales_type /* oq_nbits_type */,
                               const void* zero_points, int32_t zero_points_type, const void* bias, int32_t flags, void* Y, int64_t ldy,
                               void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_NBITS_DECODE_H */
