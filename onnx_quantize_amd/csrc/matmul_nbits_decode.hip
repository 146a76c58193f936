// The decode route of com.microsoft::MatMulNBits (include/oq_hip_nbits_decode.h): M = 1 ... 16 rows of A against the
// packed blob, which is streamed ONCE from global memory straight into registers in 16-byte loads and never passes through LDS.
//
//       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
//
//   block     256 threads; a slice of kDecodeSlice = 1024 k (blockIdx.x % splits) and rows_per_block rows of B (decode_plan.hpp).
//   A         the slice of all M rows is staged once per workgroup into LDS as fp32 (exact from fp16 / bf16; rows >= M and k >= K are
//             zeros), laid out [row][step][lane][4] so that the lanes of a wave read consecutive 16 bytes (no bank conflict).
//   lane      LK = 32 (4 bits) / 64 (8 bits) lanes lie along k, each owning 16 bytes of a row of B = 32 / 16 consecutive k; the other
//             256 / LK threads take other rows (a pass).  R rows are in flight per lane: their 16-byte loads, scales and zero points
//             are issued a whole iteration ahead of their use (the wait for them comes after the arithmetic of the previous R rows),
//             and one LDS read of A serves all R of them.
//   units     16 consecutive k lie in one group (g is a multiple of 16): d = float(q) - zp, acc = fma(a, d, acc) 16 times, then
//             sum = fma(acc, scale, sum).  zp may be fractional (HQQ): d is then rounded once, nothing else changes.
//   reduce    the R x MT sums of a lane are added across the LK lanes by a transposing butterfly (lane c ends up with value c): a
//             fixed order, log2(LK) additions per value, about one shuffle per value.
//   split K   splits > 1: the sums go to slab `split`; nbits_decode_reduce_kernel adds the slabs in slab order and finishes.  No
//             atomics, no workgroup waits on another.
//   guards    rows >= N are never loaded or written; a 16-byte load that would leave its row of B (a row of an odd number of 16-k
//             units at 4 bits is 8 bytes short of it and 8-byte aligned) is two guarded 8-byte loads; k >= K meets a zero of A.
// The 8- and 16-row tiers of a node whose groups are whole wave spans run nbits_decode_mma_kernel (further down) instead: the same
// streaming, the products on the matrix cores.
// Built with -fno-slp-vectorize (_build.py), like matmul_nbits.hip and for its reason: no v_pk_fma_f32 folds (docs/LAB_NOTES_r22.md).
// Shared: the matrix-core operand, the decoders of the blob and of a packed zero point and the checks of a call with matmul_nbits.hip
// (nbits_common.hpp); the row tiers and the butterfly with qlinear_decode.hip (decode_plan.hpp, lanes_reduce.hpp).
#include "decode_plan.hpp"
#include "lanes_reduce.hpp"
#include "nbits_common.hpp"

#include "../../include/oq_hip_nbits_decode.h"

#include <cmath>
#include <type_traits>

namespace oq {
namespace {

enum ZpKind : int32_t { kZpNone = 0, kZpPacked = 1, kZpF32 = 2, kZpF16 = 3, kZpBF16 = 4 };

struct DecodeArgs {
    const void* A;
    int32_t atype, a_vec;     // a_vec: four consecutive elements of any row can be loaded at once
    int64_t lda;
    const uint8_t* B;
    int64_t row_bytes;        // of a row of B: blocks * g * bits / 8
    int32_t b_vec;            // rows of B are whole 16-byte chunks
    const void* scales;
    int32_t scales_type;
    const void* zp;
    int32_t zp_kind;
    const void* bias;
    void* Y;
    int64_t ldy;
    float* slab;              // split K: [splits, M, N]
    int64_t M, N, K, blocks, splits, rows_per_block;
    uint32_t g;
};

__device__ __forceinline__ float typed(uint32_t raw, int32_t type) {      // a loaded fp32 word / 2-byte element as fp32
    return type == OQ_NBITS_F32 ? __uint_as_float(raw) : type == OQ_NBITS_F16 ? ElemF16::one(static_cast<uint16_t>(raw)) : ElemBF16::one(static_cast<uint16_t>(raw));
}
__device__ __forceinline__ uint32_t load_typed(const void* base, int64_t i, int32_t type) {
    return type == OQ_NBITS_F32 ? static_cast<const uint32_t*>(base)[i] : static_cast<const uint16_t*>(base)[i];
}

// the one rounding: fp32 sum -> + bias -> Y's type
__device__ __forceinline__ void finish(const DecodeArgs& p, int64_t m, int64_t n, float v) {
    if (p.bias) v += typed(load_typed(p.bias, n, p.atype), p.atype);
    if (p.atype == OQ_NBITS_F32) static_cast<float*>(p.Y)[m * p.ldy + n] = v;
    else if (p.atype == OQ_NBITS_F16) static_cast<uint16_t*>(p.Y)[m * p.ldy + n] = __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
    else static_cast<uint16_t*>(p.Y)[m * p.ldy + n] = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

// four elements of row m of A from column k on, as fp32; zeros past K
__device__ __forceinline__ f32x4 load_a4(const DecodeArgs& p, int64_t m, int64_t k) {
    f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
    if (k >= p.K) return v;
    const int64_t at = m * p.lda + k;
    if (p.a_vec && k + 4 <= p.K) {
        if (p.atype == OQ_NBITS_F32) return *reinterpret_cast<const f32x4*>(static_cast<const float*>(p.A) + at);
        const u32x2 w = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(p.A) + at);
        float e0, e1, e2, e3;
        if (p.atype == OQ_NBITS_F16) ElemF16::two(w[0], e0, e1), ElemF16::two(w[1], e2, e3);
        else ElemBF16::two(w[0], e0, e1), ElemBF16::two(w[1], e2, e3);
        return f32x4{e0, e1, e2, e3};
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < p.K) v[e] = typed(load_typed(p.A, at + e, p.atype), p.atype);
    return v;
}

template <int BITS, int MT, int R>
__global__ __launch_bounds__(kDecodeThreads) void nbits_decode_kernel(const DecodeArgs p) {
    constexpr int VAL = 128 / BITS;                  // k of a lane's 16 bytes
    constexpr int LK = kDecodeSlice / VAL;           // lanes along k
    constexpr int RP = kDecodeThreads / LK;          // rows of a pass
    constexpr int UNITS = VAL / 16, STEPS = VAL / 4;
    static_assert(R * MT <= LK && ((R * MT) & (R * MT - 1)) == 0, "the transposing reduce leaves value c in lane c");
    static_assert(kDecodeRowUnit % (RP * R) == 0, "a workgroup's rows are whole iterations");
    __shared__ __attribute__((aligned(16))) float lds_a[MT * kDecodeSlice];

    const int tid = threadIdx.x;
    const int64_t split = blockIdx.x % p.splits, row_block = blockIdx.x / p.splits;
    const int64_t k0 = split * kDecodeSlice;
    {
        const int kl = tid * 4, cs = kl / VAL, js = (kl % VAL) / 4;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
            if (m < p.M) v = load_a4(p, m, k0 + kl);
            *reinterpret_cast<f32x4*>(&lds_a[((m * STEPS + js) * LK + cs) * 4]) = v;
        }
    }
    __syncthreads();

    const int c = tid % LK, rp = tid / LK;
    const int64_t kc = k0 + static_cast<int64_t>(c) * VAL;
    const int64_t byte_off = kc * BITS / 8;
    int64_t kb[UNITS];
    bool live[UNITS];
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
        const int64_t ku = kc + 16 * u;
        live[u] = ku < p.K;
        kb[u] = live[u] ? static_cast<int64_t>(static_cast<uint32_t>(ku) / p.g) : 0;
    }
    const float zp_default = static_cast<float>(1 << (BITS - 1));

    struct Stage {
        u32x4 b[R];
        uint32_t s[R][UNITS], z[R][UNITS];
    };
    auto load = [&](Stage& st, int64_t row0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t n = row0 + r * RP + rp;
            st.b[r] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < UNITS; ++u) st.s[r][u] = st.z[r][u] = 0u;
            if (n >= p.N || !live[0]) continue;
            const uint8_t* src = p.B + n * p.row_bytes + byte_off;
            if (p.b_vec) {
                st.b[r] = *reinterpret_cast<const u32x4*>(src);
            } else {
                const u32x2 lo = *reinterpret_cast<const u32x2*>(src);
                u32x2 hi{0u, 0u};
                if (byte_off + 8 < p.row_bytes) hi = *reinterpret_cast<const u32x2*>(src + 8);
                st.b[r] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                if (!live[u]) continue;
                st.s[r][u] = load_typed(p.scales, n * p.blocks + kb[u], p.scales_type);
                if (p.zp_kind == kZpPacked) {
                    st.z[r][u] = zp_byte<BITS>(static_cast<const uint8_t*>(p.zp), n, p.blocks, kb[u]);
                } else if (p.zp_kind != kZpNone) {
                    st.z[r][u] = load_typed(p.zp, n * p.blocks + kb[u], p.zp_kind - kZpF32);
                }
            }
        }
    };

    const int64_t n_begin = row_block * p.rows_per_block, n_end = min(p.N, n_begin + p.rows_per_block);
    Stage cur, nxt;
    load(cur, n_begin);
    for (int64_t row0 = n_begin; row0 < n_end; row0 += RP * R) {
        nxt = cur;
        if (row0 + RP * R < n_end) load(nxt, row0 + RP * R);
        // A's slice does not change, so the compiler would keep ALL of it in registers across this loop: right for one row (32
        // registers), a spill to scratch from 8 rows on.  Past one row the LDS reads stay where they are written.
        if constexpr (MT > 1) asm volatile("" ::: "memory");

        float sum[R * MT];
#pragma unroll
        for (int i = 0; i < R * MT; ++i) sum[i] = 0.0f;
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
            float zpf[R], sc[R], acc[R * MT];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool have = live[u] && row0 + r * RP + rp < p.N;
                sc[r] = have ? typed(cur.s[r][u], p.scales_type) : 0.0f;
                float z = zp_default;
                if (p.zp_kind == kZpPacked) z = static_cast<float>(zp_of_byte<BITS>(cur.z[r][u], kb[u]));
                else if (p.zp_kind != kZpNone) z = typed(cur.z[r][u], p.zp_kind - kZpF32);
                zpf[r] = have ? z : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < R * MT; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = u * 4 + jj;                      // the step: k = kc + 4 j ... + 3
                f32x4 a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const f32x4*>(&lds_a[((m * STEPS + j) * LK + c) * 4]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float d[4];
                    const uint32_t w = cur.b[r][4 * j * BITS / 32];      // the word of the step's four values, and where they begin in it
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = stored<BITS>(w, 4 * j % (32 / BITS) + e) - zpf[r];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[r * MT + m] = __builtin_fmaf(a[m][e], d[e], acc[r * MT + m]);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < MT; ++m) sum[r * MT + m] = __builtin_fmaf(acc[r * MT + m], sc[r], sum[r * MT + m]);
        }

        lanes_reduce<R * MT, 1, LK>(sum, c);
        if (c < R * MT) {
            const int64_t m = c % MT, n = row0 + (c / MT) * RP + rp;
            if (m < p.M && n < p.N) {
                if (p.slab) p.slab[(split * p.M + m) * p.N + n] = sum[0];
                else finish(p, m, n, sum[0]);
            }
        }
        cur = nxt;
    }
}

// ---- the 8- and 16-row tiers on the matrix cores, where a group is a whole number of wave spans (g % (512 / BITS) == 0)
//
// 16 rows on the vector ALU are 16 fused multiply-adds per weight and an LDS read of A per four of them: the tier is bound by both at
// once.  v_mfma_f32_16x16x32_f16 / _bf16 takes the 16 rows as its A operand.  The blob still goes straight from global memory into
// registers in 16-byte loads and is dequantized there; what changes is who multiplies.
//   wave      a tile of 16 rows of B (lane & 15) over the 1024 k of the slice; lane (c, qd = lane >> 4) loads the 16 bytes at
//             k = SP s + VAL qd of span s (SP = 4 VAL = 128 / 64 k): all 8 / 16 spans of a tile are in flight at once, and those of the
//             next tile are issued before the arithmetic of this one.
//   MFMA j    of a span takes the lane's j-th eight values: k = SP s + VAL qd + 8 j ... + 7 -- the VAL / 8 MFMAs of a span cover it
//             exactly, in an order A's fragments follow.  The span lies in one group, so its sum is folded with one scale.
//   B         q - zp for integer zero points: an exact fp16 / bf16 operand, as in matmul_nbits.hip.  Float zero points (HQQ): the
//             operand is q, and the span's sum is corrected by zp * rowsum(A) -- the row sums come from the same MFMAs against a
//             fragment of ones.
//   A         LDS holds the slice as 2-byte operands, rows padded by 16 bytes (16 lanes x 16 bytes: every bank once).  fp16 and bf16
//             as they are; fp32 as THREE bf16 pieces, a = b1 + b2 + b3 exactly (3 x 8 significand bits, bf16 has fp32's range: no row
//             scale, rows at 1e30 and 1e-30 alike), each piece times an 8-bit integer exact in fp32.
constexpr int kMmaRow = kDecodeSlice * 2 + 16;      // bytes of a row of A in LDS

template <int ATYPE, int BITS>
__global__ __launch_bounds__(kDecodeThreads) void nbits_decode_mma_kernel(const DecodeArgs p) {
    typedef std::conditional_t<ATYPE == OQ_NBITS_F16, OpF16, OpBF16> OP;
    typedef typename OP::frag frag;
    constexpr int PIECES = ATYPE == OQ_NBITS_F32 ? 3 : 1;
    constexpr int VAL = 128 / BITS, SP = 4 * VAL, NS = kDecodeSlice / SP, NJ = VAL / 8;
    __shared__ __attribute__((aligned(16))) unsigned char lds_a[PIECES * 16 * kMmaRow];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, qd = lane >> 4;
    const int64_t split = blockIdx.x % p.splits, row_block = blockIdx.x / p.splits;
    const int64_t k0 = split * kDecodeSlice;
    {
        const int kl = tid * 4;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
            if (m < p.M) v = load_a4(p, m, k0 + kl);
#pragma unroll
            for (int piece = 0; piece < PIECES; ++piece) {
                uint16_t h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    h[e] = OP::round(v[e]);
                    if constexpr (PIECES > 1) {      // what the piece left; an infinity stays in the first piece alone
                        const float took = ElemBF16::one(h[e]);
                        v[e] = fabsf(took) < INFINITY ? v[e] - took : 0.0f;
                    }
                }
                *reinterpret_cast<u32x2*>(lds_a + (piece * 16 + m) * kMmaRow + kl * 2) = u32x2{h[0] | (uint32_t(h[1]) << 16), h[2] | (uint32_t(h[3]) << 16)};
            }
        }
    }
    __syncthreads();

    const bool float_zp = p.zp_kind >= kZpF32;
    const uint32_t steps_per_group = p.g / SP;
    const uint32_t step0 = static_cast<uint32_t>(k0 / SP);
    const uint32_t kb0 = step0 / steps_per_group;
    const uint32_t rem0 = step0 % steps_per_group;
    const int64_t byte_off = (k0 + static_cast<int64_t>(VAL) * qd) * BITS / 8;      // + 64 s: the lane's 16 bytes of span s
    const int64_t n_begin = row_block * p.rows_per_block, n_end = min(p.N, n_begin + p.rows_per_block);
    const unsigned char* const a_frag = lds_a + c * kMmaRow + qd * VAL * 2;
    const frag ones = __builtin_bit_cast(frag, u32x4{OP::kOnes, OP::kOnes, OP::kOnes, OP::kOnes});

    struct Stage {
        u32x4 b[NS];
        uint32_t s[NS], z[NS];
    };
    auto load = [&](Stage& st, int64_t n) {
        uint32_t kb = kb0, rem = rem0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            st.b[s] = u32x4{0u, 0u, 0u, 0u};
            st.s[s] = st.z[s] = 0u;
            if (n < p.N && k0 + s * SP < p.K) {
                if (k0 + s * SP + VAL * qd < p.K) st.b[s] = *reinterpret_cast<const u32x4*>(p.B + n * p.row_bytes + byte_off + s * 64);
                st.s[s] = load_typed(p.scales, n * p.blocks + kb, p.scales_type);
                if (p.zp_kind == kZpPacked) {
                    st.z[s] = zp_of_byte<BITS>(zp_byte<BITS>(static_cast<const uint8_t*>(p.zp), n, p.blocks, kb), kb);
                } else if (p.zp_kind != kZpNone) {
                    st.z[s] = load_typed(p.zp, n * p.blocks + kb, p.zp_kind - kZpF32);
                }
            }
            if (++rem == steps_per_group) rem = 0, ++kb;
        }
    };

    // 4 bits: the 8 loads of the next tile are issued before the arithmetic of this one.  8 bits: a tile's 16 loads are all in flight at
    // once and a second set of them does not fit the register file.
    constexpr bool kAhead = BITS == 4;
    Stage cur, nxt;
    if constexpr (kAhead) load(cur, n_begin + wave * 16 + c);
    for (int64_t t0 = n_begin + wave * 16; t0 < n_end; t0 += 64) {      // the tile: rows t0 ... t0 + 15 of B
        if constexpr (kAhead) {
            nxt = cur;
            if (t0 + 64 < n_end) load(nxt, t0 + 64 + c);
        } else {
            load(cur, t0 + c);
        }
        asm volatile("" ::: "memory");      // A's fragments are read where they are used, not kept in registers across the tiles

        const int64_t n = t0 + c;
        f32x4 sum{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (k0 + s * SP >= p.K) break;
            const float sc = n < p.N ? typed(cur.s[s], p.scales_type) : 0.0f;
            float zi = static_cast<float>(1 << (BITS - 1)), zf = 0.0f;      // the operand is q - zi; the span's sum loses zf * rowsum(A)
            if (p.zp_kind == kZpPacked) zi = static_cast<float>(cur.z[s]);
            else if (float_zp) zi = 0.0f, zf = n < p.N ? typed(cur.z[s], p.zp_kind - kZpF32) : 0.0f;
            f32x4 acc{0.0f, 0.0f, 0.0f, 0.0f}, asum{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                uint32_t d[4];      // the lane's j-th eight values: one word at 4 bits, two at 8
#pragma unroll
                for (int h = 0; h < BITS / 4; ++h) dequant_word<OP, BITS>(cur.b[s][j * BITS / 4 + h], zi, d + h * (16 / BITS));
                const frag b = __builtin_bit_cast(frag, u32x4{d[0], d[1], d[2], d[3]});
#pragma unroll
                for (int piece = 0; piece < PIECES; ++piece) {
                    const frag a = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(a_frag + piece * 16 * kMmaRow + (s * SP + 8 * j) * 2));
                    acc = OP::mma(a, b, acc);
                    if (float_zp) asum = OP::mma(a, ones, asum);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[r] = __builtin_fmaf(__builtin_fmaf(-zf, asum[r], acc[r]), sc, sum[r]);
        }

        // C/D map of the 16x16 MFMAs: column = lane & 15 (the row of B), row = 4 (lane >> 4) + r (the row of A)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = 4 * qd + r;
            if (m < p.M && n < p.N) {
                if (p.slab) p.slab[(split * p.M + m) * p.N + n] = sum[r];
                else finish(p, m, n, sum[r]);
            }
        }
        if constexpr (kAhead) cur = nxt;
    }
}

// the slabs of a split K, added in slab order
__global__ __launch_bounds__(kDecodeThreads) void nbits_decode_reduce_kernel(const DecodeArgs p) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kDecodeThreads + threadIdx.x;
    if (i >= p.M * p.N) return;
    float v = p.slab[i];
    for (int64_t s = 1; s < p.splits; ++s) v += p.slab[s * p.M * p.N + i];
    finish(p, i / p.N, i % p.N, v);
}

// ---- host
struct Plan : DecodePlan {      // and the workspace: include/oq_hip_nbits_decode.h, `workspace`
    float* slab;
};

constexpr NbitsRoute kRoute{"oq_matmul_nbits_decode", kDecodeMaxRows, 16, "a lane's unit of 16 k would straddle two groups", true};

Plan make_plan(int64_t M, int64_t K, int64_t N, int32_t atype, Workspace& ws) {
    Plan pl{make_decode_plan(M, K, N, atype == OQ_NBITS_F32)};
    pl.slab = ws.take<float>(pl.slab_bytes);
    return pl;
}

// the 8- and 16-row tiers of a node whose groups are whole wave spans: the matrix cores
bool mma_route(const Plan& pl, int32_t bits, int64_t g) { return pl.tier >= 8 && g % (512 / bits) == 0; }

template <int BITS>
void launch(const DecodeArgs& p, const Plan& pl, hipStream_t s) {
    if (mma_route(pl, BITS, p.g)) {
        const unsigned grid = static_cast<unsigned>(pl.grid);
        if (p.atype == OQ_NBITS_F16) nbits_decode_mma_kernel<OQ_NBITS_F16, BITS><<<grid, kDecodeThreads, 0, s>>>(p);
        else if (p.atype == OQ_NBITS_BF16) nbits_decode_mma_kernel<OQ_NBITS_BF16, BITS><<<grid, kDecodeThreads, 0, s>>>(p);
        else nbits_decode_mma_kernel<OQ_NBITS_F32, BITS><<<grid, kDecodeThreads, 0, s>>>(p);
        return;
    }
    with_decode_tier(pl.tier, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        constexpr int R = MT == 16 ? 2 : 4;
        nbits_decode_kernel<BITS, MT, R><<<static_cast<unsigned>(pl.grid), kDecodeThreads, 0, s>>>(p);
    });
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_nbits_decode_extension_version(void) { return OQ_NBITS_DECODE_EXTENSION_VERSION; }

size_t oq_matmul_nbits_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype) {
    if (!type_ok(atype) || !shape_ok(M, K, N, group_size) || M > kDecodeMaxRows || group_size % 16 != 0) {
        set_error("oq_matmul_nbits_decode_workspace_bytes: M=%lld K=%lld N=%lld group_size=%lld atype=%d outside the bounds of the decode route",
                  (long long)M, (long long)K, (long long)N, (long long)group_size, atype);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, atype, ws);
    return ws.total();
}

int32_t oq_matmul_nbits_decode(const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, const void* B, int32_t bits, int64_t N,
                               int64_t group_size, const void* scales, int32_t scales_type, const void* zero_points, int32_t zero_points_type,
                               const void* bias, int32_t flags, void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = kRoute.fn;
    int32_t st = operands_ok(fn, A, B, scales, Y, atype, scales_type);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(zero_points_type == OQ_NBITS_ZP_PACKED_U8 || zero_points_type == OQ_NBITS_F32 || zero_points_type == atype, OQ_ERR_INVALID_ARGUMENT,
               "%s: zero_points_type %d is neither packed uint8 (%d), fp32 nor atype %d", fn, zero_points_type, OQ_NBITS_ZP_PACKED_U8, atype);
    st = extents_and_flags_ok(kRoute, M, K, N, lda, ldy, bits, group_size, flags);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(!(flags & OQ_NBITS_FLOAT_ZERO_POINTS) || zero_points_type != OQ_NBITS_ZP_PACKED_U8, OQ_ERR_INVALID_ARGUMENT,
               "%s: flags say float zero points, zero_points_type says packed uint8", fn);
    OQ_REQUIRE(shape_ok(M, K, N, group_size), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld group_size=%lld: an operand beyond 2^40 elements", fn,
               (long long)M, (long long)K, (long long)N, (long long)group_size);
    const uintptr_t elem = atype == OQ_NBITS_F32 ? 4 : 2;
    const uintptr_t zp_elem = zero_points_type == OQ_NBITS_ZP_PACKED_U8 ? 1 : zero_points_type == OQ_NBITS_F32 ? 4 : 2;
    OQ_REQUIRE(aligned_to(A, elem) && aligned_to(Y, elem) && aligned_to(bias, elem) && aligned_to(scales, scales_type == OQ_NBITS_F32 ? 4 : 2) &&
                   aligned_to(zero_points, zp_elem),
               OQ_ERR_INVALID_ARGUMENT, "%s: A, Y, bias, scales and zero_points must be aligned to their element", fn);
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, atype, ws);
    st = blob_and_workspace_ok(fn, B, ws, workspace, workspace_bytes);
    if (st != OQ_OK) return st;

    hipStream_t s = as_stream(stream);
    DecodeArgs p{};
    p.A = A, p.atype = atype, p.lda = lda;
    p.a_vec = lda % 4 == 0 && aligned_to(A, 4 * elem);
    p.B = static_cast<const uint8_t*>(B);
    p.blocks = ceil_div(K, group_size);
    p.row_bytes = p.blocks * group_size * bits / 8;
    p.b_vec = p.row_bytes % 16 == 0;
    p.scales = scales, p.scales_type = scales_type;
    p.zp = zero_points;
    p.zp_kind = !zero_points ? kZpNone : zero_points_type == OQ_NBITS_ZP_PACKED_U8 ? kZpPacked : kZpF32 + zero_points_type;
    p.bias = bias;
    p.Y = Y, p.ldy = ldy;
    p.slab = pl.slab;
    p.M = M, p.N = N, p.K = K, p.splits = pl.splits, p.rows_per_block = pl.rows_per_block;
    p.g = static_cast<uint32_t>(group_size);
    if (bits == 4) launch<4>(p, pl, s);
    else launch<8>(p, pl, s);
    st = check_launch("nbits_decode_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    nbits_decode_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kDecodeThreads)), kDecodeThreads, 0, s>>>(p);
    return check_launch("nbits_decode_reduce_kernel");
}

}  // extern "C"
