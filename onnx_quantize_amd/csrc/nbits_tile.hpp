// What the tile GEMMs on the exact (q - zp) matrix-core operand share (matmul_nbits.hip: B is the MatMulNBits blob; qdq_matmul.hip:
// W is a [K, N] byte matrix): the argument block, the one rounding of a sum to Y's type, the guarded load
// of eight elements of A, the body of the GEMM kernel (tile_gemm), the kernel that adds the slabs of a split K, the kernel that
// splits an fp32 A into two fp16 pieces, the plan with its workspace, and the host tail of a call.  matmul_nbits.hip's GEMM kernel
// is tile_gemm with the file's staging policy: how B reaches LDS and where a fragment finds it there, and nothing else; so is
// matmul_nbits_fzp.hip's (float zero points), whose policy also switches on the row sums of A and their correction.
// qdq_matmul.hip's is a written-out copy of the same body with its staging in place: built on tile_gemm, its fp32-A kernel of the
// 128-row tile measured 0.4 - 3 % slower at M = 2048, twice (docs/LAB_NOTES_r30.md).  A fix to the body is made in both.
//
//   block     256 threads = 2 x 2 waves; tile 32 * MT rows (MT = 4: 128; MT = 1: 32, for M <= 32) x 128 columns; k-step 64.
//   wave      16 * MT x 64 outputs = MT x 4 MFMA tiles; per tile 4 fp32 of the group accumulator and 4 of the running sum.
//   operands  both have k as their fast axis in LDS, which is what the 16x16x32 lane map wants (lane l: row / column l & 15,
//             k = 8 (l >> 4) ... + 7): a 16-byte ds_read per fragment, rows padded to 144 bytes (conflict-free).
//   staging   registers: the global loads of step i + 1 are issued before the MFMAs of step i; one LDS buffer, two barriers a step.
//   fp32 A    nbits_split_rows_kernel writes two fp16 pieces per element under one power-of-two scale per row (the row's largest
//             lands in [2^14, 2^15)): hi = fp16(x s), lo = fp16((x s - hi) 2^11).  lo meets B 2^-11 (exact: |q - zp| >= 1 keeps
//             it a normal fp16), so both products share the accumulator.  A hi that would be an fp16 subnormal is dropped into lo.
//   split K   few output tiles (small M): blockIdx.y takes a range of k-steps, writes its sum to slab y; nbits_reduce_kernel adds
//             the slabs in slab order and finishes.  No atomics anywhere.
//   guards    every global access is guarded by M, N, K: rows >= M, columns >= N and k >= K are zeros in LDS (A) or never read
//             (scales); how a policy keeps its reads of B and of the zero points inside the operand is said where it reads them.
#pragma once

#include "nbits_common.hpp"
#include "tile_plan.hpp"

#include <cmath>

namespace oq {
namespace {

constexpr int kRow = kBK * 2 + 16;   // bytes of a tile row in LDS (kBK: two MFMA depths): 16 lanes x 16 bytes land in 16 different bank quads

struct NbitsArgs {
    const uint16_t* A;      // 2-byte operand: A itself, or the hi pieces
    const uint16_t* A_lo;   // fp32 A: the lo pieces
    int64_t lda, Ka;        // Ka: columns of A that exist (K; the pieces: K padded to 8, zero-filled)
    int32_t a_vec;          // rows of A are 16-byte aligned
    const uint8_t* B;
    const void* scales;
    int32_t scales_f32;
    const uint8_t* zp;
    const void* bias;
    const int32_t* row_exp; // fp32 A: Y row m = sum * 2^row_exp[m]
    void* Y;
    int64_t ldy;
    float* slab;            // split K: [splits, M, N]
    int64_t M, N, K, g, blocks, tiles_m, steps_per_split;
};

// ---- the one rounding: fp32 sum -> (row scale) -> + bias -> Y's type.  OUT: an oq_nbits_type
template <int OUT>
__device__ __forceinline__ void finish(const NbitsArgs& p, int64_t m, int64_t n, float v) {
    typedef std::conditional_t<OUT == OQ_NBITS_BF16, OpBF16, OpF16> OP;
    if constexpr (OUT == OQ_NBITS_F32) {
        v = ldexpf(v, p.row_exp[m]);
        if (p.bias) v += static_cast<const float*>(p.bias)[n];
        static_cast<float*>(p.Y)[m * p.ldy + n] = v;
    } else {
        if (p.bias) v += OP::one(static_cast<const uint16_t*>(p.bias)[n]);
        static_cast<uint16_t*>(p.Y)[m * p.ldy + n] = OP::round(v);
    }
}

// eight 2-byte elements of row `row` from column k on; zeros past Ka
__device__ __forceinline__ u32x4 load_a8(const uint16_t* row, int64_t k, int64_t Ka, bool vec) {
    if (vec && k + 8 <= Ka) return *reinterpret_cast<const u32x4*>(row + k);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t e0 = (k + 2 * j < Ka) ? row[k + 2 * j] : 0u;
        const uint32_t e1 = (k + 2 * j + 1 < Ka) ? row[k + 2 * j + 1] : 0u;
        w[j] = e0 | (e1 << 16);
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// 32 stored values (k ascending) minus the zero point -> 32 exact 2-byte operands
template <typename OP, int BITS>
__device__ __forceinline__ void dequant32(const u32x4 (&raw)[BITS / 4], float zpf, u32x4 (&out)[4]) {
    uint32_t d[16];
#pragma unroll
    for (int wi = 0; wi < BITS; ++wi) dequant_word<OP, BITS>(raw[wi >> 2][wi & 3], zpf, d + wi * (16 / BITS));
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = u32x4{d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]};
}

// ---- the GEMM.  Stage, a file's staging policy (BlobStage<BITS> of matmul_nbits.hip, FzpStage<BITS> of matmul_nbits_fzp.hip), holds
// what one thread has loaded of the next k-step of B:
//   args                        the kernel's argument block, an NbitsArgs or a struct derived from it
//   kRows, kFragStride          rows of the policy's LDS image of B; rows between a lane's fragments nt and nt + 1
//   frag_row(wn, lane)          the image row of the lane's fragment nt = 0 in column half wn
//   group(p, k), within(p, k)   the k-group of a k and k's place inside it
//   Stage(p, tid, n0)           which part of the 64 x 128 step of B this thread stages
//   load(p, k, k_begin, k_end)  global memory -> registers, for the step at k of the block's range [k_begin, k_end)
//   store<OP>(p, lds_b)         registers -> (q - zp) as 2-byte operands in the image
//   kFloatZp                    the zero points are floating point (matmul_nbits_fzp.hip): the operand is q - zi,
//                               zi = rint(zp) clamped, and a group's sum loses f * rowsum(A), f = zp - zi.  The row sums rs come from
//                               one more MFMA per fragment of A, against a fragment of ones: they land in exactly the rows a lane's
//                               accumulators hold.  Every line of it is under `if constexpr`: with kFloatZp false the body compiles
//                               to the text it had without it (scripts/compare_kernel_asm.py).
//   group_terms(s, wn, lane,    kFloatZp: the f and the scales of the lane's four columns, for the group of MFMA depth s of the stored
//               f, sc)          step.  The policy stages the scale with the zero point and hands both over through LDS, so the body
//                               loads no scales of its own: four registers, and their addresses, that the row sums need
template <int OUT, int MT, typename Stage>
__device__ __forceinline__ void tile_gemm(const typename Stage::args& p) {
    typedef std::conditional_t<OUT == OQ_NBITS_BF16, OpBF16, OpF16> OP;
    typedef typename OP::frag frag;
    constexpr int PIECES = OUT == OQ_NBITS_F32 ? 2 : 1;
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = PIECES * BM * 8 / kThreads;      // 16-byte chunks of the A tile(s) per thread: PIECES * MT
    __shared__ __attribute__((aligned(16))) unsigned char lds[(PIECES * BM + Stage::kRows) * kRow];
    unsigned char* const lds_b = lds + PIECES * BM * kRow;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x % p.tiles_m) * BM;
    const int64_t n0 = static_cast<int64_t>(blockIdx.x / p.tiles_m) * kBN;
    const int64_t k_begin = static_cast<int64_t>(blockIdx.y) * p.steps_per_split * kBK;
    const int64_t k_end = min(p.K, k_begin + p.steps_per_split * kBK);

    // what this thread stages: A_CHUNKS chunks of A, and the policy's part of B
    u32x4 a_regs[A_CHUNKS];
    Stage b_stage(p, tid, n0);

    auto load_step = [&](int64_t k) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            const int piece = id / (BM * 8), r = (id >> 3) % BM, kc = id & 7;
            const int64_t m = m0 + r;
            const uint16_t* base = (PIECES == 2 && piece == 1) ? p.A_lo : p.A;
            a_regs[i] = (m < p.M && k + kc * 8 < p.Ka) ? load_a8(base + m * p.lda, k + kc * 8, p.Ka, p.a_vec != 0) : u32x4{0u, 0u, 0u, 0u};
        }
        b_stage.load(p, k, k_begin, k_end);
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            *reinterpret_cast<u32x4*>(lds + (id >> 3) * kRow + (id & 7) * 16) = a_regs[i];      // id >> 3 = piece * BM + r
        }
        b_stage.template store<OP>(p, lds_b);
    };

    f32x4 sum[MT][NT], acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sum[mt][nt] = acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 rs[Stage::kFloatZp ? MT : 1];      // kFloatZp: the sums of A's rows over the k that acc has seen
    const frag ones = __builtin_bit_cast(frag, u32x4{OP::kOnes, OP::kOnes, OP::kOnes, OP::kOnes});
    if constexpr (Stage::kFloatZp) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) rs[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const int64_t col = n0 + wn * 64 + (lane & 15);          // + 16 nt: the output column of this lane in tile nt
    auto load_scales = [&](int64_t kb, float (&sc)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t n = col + 16 * nt;
            sc[nt] = 0.0f;
            if (n < p.N) sc[nt] = p.scales_f32 ? static_cast<const float*>(p.scales)[n * p.blocks + kb] : OP::one(static_cast<const uint16_t*>(p.scales)[n * p.blocks + kb]);
        }
    };
    float sc[NT];
    int64_t in_group = Stage::within(p, k_begin);      // k of the next MFMA depth inside its group
    if constexpr (!Stage::kFloatZp)
        if (k_begin < k_end) load_scales(Stage::group(p, k_begin), sc);

    const unsigned char* const a_frag = lds + (wm * 16 * MT + (lane & 15)) * kRow + (lane >> 4) * 16;
    const unsigned char* const b_frag = lds_b + Stage::frag_row(wn, lane) * kRow + (lane >> 4) * 16;

    if (k_begin < k_end) load_step(k_begin);
    for (int64_t k = k_begin; k < k_end; k += kBK) {
        store_step();
        __syncthreads();
        if (k + kBK < k_end) load_step(k + kBK);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t ks = k + 32 * s;
            if (ks < k_end) {
                frag b[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b[nt] = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(b_frag + nt * Stage::kFragStride * kRow + s * 64));
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const frag a = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(a_frag + mt * 16 * kRow + s * 64));
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = OP::mma(a, b[nt], acc[mt][nt]);
                    if constexpr (Stage::kFloatZp) rs[mt] = OP::mma(a, ones, rs[mt]);
                }
                if constexpr (PIECES == 2) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b[nt] = b[nt] * static_cast<_Float16>(0.00048828125f);      // 2^-11, exact
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const frag a = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(a_frag + (BM + mt * 16) * kRow + s * 64));
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = OP::mma(a, b[nt], acc[mt][nt]);
                        if constexpr (Stage::kFloatZp) rs[mt] = OP::mma(a, ones * static_cast<_Float16>(0.00048828125f), rs[mt]);
                    }
                }
                in_group += 32;
                // The fold is one scalar fma per output element: the files that hold this body are built with -fno-slp-vectorize, paired
                // (v_pk_fma_f32) it gave wrong sums on the MI355X (docs/LAB_NOTES_r22.md).
                if (in_group == p.g || ks + 32 >= k_end) {      // the group (or this block's part of it) is complete
                    if constexpr (Stage::kFloatZp) {            // acc holds sum a (q - zi): what f * sum a takes away is still missing
                        float fz[NT];
                        Stage::group_terms(s, wn, lane, fz, sc);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                                for (int r = 0; r < 4; ++r) acc[mt][nt][r] = __builtin_fmaf(-fz[nt], rs[mt][r], acc[mt][nt][r]);
                            rs[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                        }
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) sum[mt][nt][r] = __builtin_fmaf(acc[mt][nt][r], sc[nt], sum[mt][nt][r]);
                            acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                        }
                    in_group = 0;
                    if constexpr (!Stage::kFloatZp)
                        if (ks + 32 < k_end) load_scales(Stage::group(p, ks + 32), sc);
                }
            }
        }
        __syncthreads();
    }

    // C/D map of the 16x16 MFMAs: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wm * 16 * MT + mt * 16 + 4 * (lane >> 4) + r, n = col + 16 * nt;
                if (m < p.M && n < p.N) {
                    if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = sum[mt][nt][r];
                    else finish<OUT>(p, m, n, sum[mt][nt][r]);
                }
            }
}

// the slabs of a split K, added in slab order
template <int OUT>
__global__ __launch_bounds__(kThreads) void nbits_reduce_kernel(const NbitsArgs p, const int splits) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= p.M * p.N) return;
    float v = p.slab[i];
    for (int s = 1; s < splits; ++s) v += p.slab[s * p.M * p.N + i];
    finish<OUT>(p, i / p.N, i % p.N, v);
}

// fp32 A -> two fp16 pieces per element and one exponent per row (one block per row)
__global__ __launch_bounds__(kThreads) void nbits_split_rows_kernel(const float* A, int64_t K, int64_t lda, int64_t Kp, uint16_t* hi, uint16_t* lo,
                                                                    int32_t* row_exp) {
    __shared__ float part[kThreads / kWave];
    const int64_t m = blockIdx.x;
    const float* row = A + m * lda;
    float mx = 0.0f;
    for (int64_t k = threadIdx.x; k < K; k += kThreads) mx = nmax(mx, fabsf(row[k]));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = nmax(nmax(part[0], part[1]), nmax(part[2], part[3]));
    int shift = 0;                               // a zero row, and a row with a NaN or an infinity (it stays what it is): unscaled
    if (mx > 0.0f && mx < INFINITY) {
        int e;
        frexpf(mx, &e);                          // mx in [2^(e-1), 2^e)  ->  scaled into [2^14, 2^15)
        shift = 15 - e;
    }
    for (int64_t k = threadIdx.x; k < Kp; k += kThreads) {
        const float xs = ldexpf(k < K ? row[k] : 0.0f, shift);
        _Float16 h = static_cast<_Float16>(xs);
        if (fabsf(static_cast<float>(h)) < 6.103515625e-05f) h = static_cast<_Float16>(0.0f);      // no fp16 subnormal reaches the matrix core as hi
        const _Float16 l = static_cast<_Float16>((xs - static_cast<float>(h)) * 2048.0f);
        hi[m * Kp + k] = __builtin_bit_cast(uint16_t, h);
        lo[m * Kp + k] = __builtin_bit_cast(uint16_t, l);
    }
    if (threadIdx.x == 0) row_exp[m] = -shift;
}

// ---- host
struct Plan : TilePlan {      // and the workspace: include/oq_hip_nbits.h, `workspace`
    int64_t kp;               // fp32 A: K padded to 8, the width of its pieces
    uint16_t *hi, *lo;        // fp32 A: its two fp16 pieces [M, kp]
    int32_t* row_exp;         // fp32 A: the scale exponent of every row
    float* slab;
};

bool tile_shape_ok(int64_t M, int64_t K, int64_t N, int64_t g) {      // and the pieces of an fp32 A
    return shape_ok(M, K, N, g) && count_ok(M * ((K + 7) / 8 * 8));
}

Plan make_plan(int64_t M, int64_t K, int64_t N, int32_t atype, Workspace& ws) {
    Plan pl{make_tile_plan(M, K, N)};
    pl.kp = (K + 7) / 8 * 8;
    const size_t piece_bytes = atype == OQ_NBITS_F32 ? static_cast<size_t>(M) * pl.kp * 2 : 0;
    pl.hi = ws.take<uint16_t>(piece_bytes);
    pl.lo = ws.take<uint16_t>(piece_bytes);
    pl.row_exp = ws.take<int32_t>(atype == OQ_NBITS_F32 ? static_cast<size_t>(M) * 4 : 0);
    pl.slab = ws.take<float>(pl.slab_bytes);
    return pl;
}

// the body of a file's workspace query: 0, after `refuse()` has set the file's message, for a type or a shape outside the bounds
template <typename Refuse>
size_t plan_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t g, int32_t atype, Refuse refuse) {
    if (!type_ok(atype) || !tile_shape_ok(M, K, N, g)) {
        refuse();
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, atype, ws);
    return ws.total();
}

// what every call fills in alike; B, g and blocks are the file's own
inline void fill_args(NbitsArgs& p, const void* scales, int32_t scales_type, const void* zero_points, const void* bias, void* Y, int64_t ldy, int64_t M,
                      int64_t N, int64_t K, const Plan& pl) {
    p.scales = scales;
    p.scales_f32 = scales_type == OQ_NBITS_F32;
    p.zp = static_cast<const uint8_t*>(zero_points);
    p.bias = bias;
    p.Y = Y;
    p.ldy = ldy;
    p.M = M, p.N = N, p.K = K;
    p.tiles_m = pl.tiles_m, p.steps_per_split = pl.steps_per_split;
    p.slab = pl.slab;
}

// an fp32 A: its pieces and row exponents into the plan's workspace; `p` then reads them as its A
inline int32_t split_rows(NbitsArgs& p, const Plan& pl, const void* A, int64_t M, int64_t K, int64_t lda, hipStream_t s) {
    nbits_split_rows_kernel<<<static_cast<unsigned>(M), kThreads, 0, s>>>(static_cast<const float*>(A), K, lda, pl.kp, pl.hi, pl.lo, pl.row_exp);
    const int32_t st = check_launch("nbits_split_rows_kernel");
    if (st != OQ_OK) return st;
    p.A = pl.hi, p.A_lo = pl.lo, p.lda = pl.kp, p.Ka = pl.kp, p.a_vec = 1, p.row_exp = pl.row_exp;
    return OQ_OK;
}

// the second launch of a split K
template <int OUT>
int32_t reduce_slabs(const NbitsArgs& p, const Plan& pl, hipStream_t s) {
    nbits_reduce_kernel<OUT><<<static_cast<unsigned>(ceil_div(p.M * p.N, kThreads)), kThreads, 0, s>>>(p, static_cast<int>(pl.splits));
    return check_launch("nbits_reduce_kernel");
}

// the tail of a call: A as the kernel reads it, then the file's `run(out)`, out an integral constant of A's oq_nbits_type
template <typename Run>
int32_t run_for_a(NbitsArgs& p, const Plan& pl, const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, hipStream_t s, Run run) {
    if (atype == OQ_NBITS_F32) {
        const int32_t st = split_rows(p, pl, A, M, K, lda, s);
        if (st != OQ_OK) return st;
        return run(std::integral_constant<int, OQ_NBITS_F32>{});
    }
    p.A = static_cast<const uint16_t*>(A), p.lda = lda, p.Ka = K, p.a_vec = aligned_to(A, 16) && lda % 8 == 0;
    return atype == OQ_NBITS_BF16 ? run(std::integral_constant<int, OQ_NBITS_BF16>{}) : run(std::integral_constant<int, OQ_NBITS_F16>{});
}

}  // namespace
}  // namespace oq
