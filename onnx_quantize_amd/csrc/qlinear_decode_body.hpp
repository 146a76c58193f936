// The decode route of the 8-bit products as bodies, for qlinear_function.hip (include/oq_hip_qlinear_function.h): the text of the
// kernels of qlinear_decode.hip, each as a __device__ __forceinline__ function that a kernel wraps (the kernel declares the LDS and
// calls the body), with two flags:
//   QA   A is fp32 and is quantized to its 8-bit type on the way into LDS (quant_k16 in the place of load_k16): the staged image, and
//        so the row sums, the products and the LDS footprint, are those of the byte route.
//   DQ   the epilogue ends in Y = (fp32(q) - fp32(y_zp)) * y_scale as fp32 instead of the 8-bit q (finish_acc).
// qlinear_decode.hip keeps its own text and does NOT include this file: wrapped around these bodies with the flags off, 18 of its 19
// kernels compile to another order of instructions and other register numbers (docs/LAB_NOTES_r32.md, section 1), and
// scripts/compare_kernel_asm.py holds that file to its text.  So the argument struct, the bodies and the plan's workspace piece
// below are a copy; the guarded loads, the quantizer, the epilogue (qlinear_epilogue.hpp), the plan (qlinear_decode_plan.hpp) and the
// butterfly (lanes_reduce.hpp) are the one shared text.  The flags stay template arguments although this file's one user sets both:
// they mark the only places where the copy departs from the original.
// What a workgroup does and why: qlinear_decode.hip.
#pragma once

#include "lanes_reduce.hpp"
#include "qlinear_decode_plan.hpp"
#include "qlinear_epilogue.hpp"

#include "../../include/oq_hip_qlinear_decode.h"

namespace oq {
namespace {

constexpr uint32_t kOnes = 0x01010101u;

struct QdArgs {
    const uint8_t* A;
    const uint8_t* B;
    int64_t lda, ldb;
    uint32_t a_flip, b_flip;       // 0x80808080 for an unsigned operand
    int32_t a_signed, b_signed;
    int32_t a_vec, b_vec;          // rows are 16-byte aligned (A, B in NK) / 4-byte aligned (B in KN)
    const float* a_scale;
    const void* a_zp;
    const float* b_scale;
    const void* b_zp;
    int32_t b_per_column;
    const int32_t* C;
    const float* y_scale;
    const void* y_zp;
    int32_t out;
    void* Y;
    int64_t ldy;
    int32_t need_rowsum;           // 0: its multiplier zb' is zero
    uint32_t* slab;                // split K: [splits, M, N]
    uint32_t M, N, K, slice, splits, cols_per_block;      // extents are below 2^31: 32-bit indices, 64-bit only where an offset is formed
};

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t acc) {
    return static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), static_cast<int>(acc), false));
}

// lds_rs[m] = the sum of the staged (flipped) slice of row m, `quads` dwords: wave w takes rows w, w + 4, ...  Ends in a barrier.
template <int MT, bool KN, int ROW = kQlDecodeSlice / 4>      // ROW: dwords from one row of the [row][k] image to the next
__device__ __forceinline__ void row_sums(const QdArgs& p, const uint32_t* lds_a, uint32_t* lds_rs, int quads, int tid) {
    const int lane = tid & 63;
    if (p.need_rowsum) {
        for (int m = tid >> 6; m < MT; m += kQlDecodeThreads / kWave) {
            uint32_t s = 0u;
            for (int q = lane; q < quads; q += kWave) s = dot4(lds_a[KN ? q * MT + m : m * ROW + q], kOnes, s);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s), off, kWave));
            if (lane == 0) lds_rs[m] = s;
        }
    } else if (tid < MT) {
        lds_rs[tid] = 0u;
    }
    __syncthreads();
}

// what a column of this launch needs: zb'[n], and -- where the launch finishes -- C[n] and the fp32 scale
__device__ __forceinline__ ColTerms decode_col(const QdArgs& p, uint32_t n) {
    ColTerms c;
    c.zb = shifted_b_zp(p, n);
    c.add = (!p.slab && p.C) ? static_cast<uint32_t>(p.C[n]) : 0u;
    c.scale = p.slab ? 0.0f : out_scale(p, n);
    return c;
}

// the slice's corrected value of (m, n): into its slab, or -- one slice -- through the epilogue
template <bool DQ>
__device__ __forceinline__ void emit(const QdArgs& p, uint32_t split, uint32_t m, uint32_t n, uint32_t S, uint32_t rs, uint32_t cs, uint32_t ks,
                                     uint32_t za, const ColTerms& c) {
    const uint32_t v = S - c.zb * rs - za * cs + ks * za * c.zb;
    if (p.slab) p.slab[(static_cast<int64_t>(split) * p.M + m) * p.N + n] = v;
    else finish_acc<DQ>(p, m, n, static_cast<int32_t>(v + c.add), c.scale);
}

constexpr int chunks_per_thread(int mt) { return (mt * (kQlDecodeSlice / 16) + kQlDecodeThreads - 1) / kQlDecodeThreads; }

// 16 raw bytes of row m of A from k on, as load_k16 delivers them; QA: quantized here from the fp32 row (p.A points at floats, lda
// counts them, a_vec says that its rows are 16-byte aligned)
template <bool QA>
__device__ __forceinline__ u32x4 stage_a16(const QdArgs& p, int m, uint32_t k) {
    if constexpr (QA) return quant_k16(reinterpret_cast<const float*>(p.A) + static_cast<int64_t>(m) * p.lda, k, p.K, p.a_vec != 0, quant_of(p), p.a_flip);
    else return load_k16(p.A + static_cast<int64_t>(m) * p.lda, k, p.K, p.a_vec != 0, p.a_flip);
}

// `lds_a`: MT * 1024 bytes, 16-byte aligned; `lds_rs`: kQlDecodeMaxRows dwords -- both declared by the kernel
template <int MT, bool CS, bool QA, bool DQ>
__device__ __forceinline__ void ql_decode_nk_body(const QdArgs& p, uint32_t* const lds_a, uint32_t* const lds_rs) {
    constexpr int R = 4;                                     // rows of B in flight per lane
    constexpr int RP = kQlDecodeThreads / kWave;             // rows of a pass: one per wave
    constexpr int LK = kQlDecodeSlice / 16;                  // lanes along k: a wave
    constexpr int CH = chunks_per_thread(MT);
    static_assert(LK == kWave && R * MT <= kWave && RP * R == kQlDecodeColUnitNK, "the transposing reduce leaves value c in lane c");

    const int tid = threadIdx.x, c = tid & 63, rp = tid >> 6;
    const uint32_t split = blockIdx.x % p.splits, col_block = blockIdx.x / p.splits;
    const uint32_t k0 = split * kQlDecodeSlice;              // below K
    const u32x4 a_flip{p.a_flip, p.a_flip, p.a_flip, p.a_flip}, b_flip{p.b_flip, p.b_flip, p.b_flip, p.b_flip};
    {
        u32x4 v[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads, m = id / LK;
            v[i] = a_flip;
            if (id < MT * LK && m < static_cast<int>(p.M)) v[i] = stage_a16<QA>(p, m, k0 + 16 * (id % LK));
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads;
            if (id < MT * LK) *reinterpret_cast<u32x4*>(&lds_a[id * 4]) = v[i] ^ a_flip;
        }
    }
    __syncthreads();
    row_sums<MT, false>(p, lds_a, lds_rs, kQlDecodeSlice / 4, tid);

    const uint32_t za = shifted_a_zp(p);
    const uint32_t ks = min(p.K, k0 + kQlDecodeSlice) - k0;
    const uint32_t n_begin = col_block * p.cols_per_block, n_end = min(p.N, n_begin + p.cols_per_block);

    struct Stage {
        u32x4 b[R];
    };
    auto load = [&](Stage& st, uint32_t row0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t n = row0 + r * RP + rp;
            st.b[r] = b_flip;
            if (n < p.N) st.b[r] = load_k16(p.B + static_cast<int64_t>(n) * p.ldb, k0 + 16 * c, p.K, p.b_vec != 0, p.b_flip);
        }
    };

    Stage cur, nxt;
    load(cur, n_begin);
    for (uint32_t row0 = n_begin; row0 < n_end; row0 += RP * R) {
        nxt = cur;
        if (row0 + RP * R < n_end) load(nxt, row0 + RP * R);
        // A's slice does not change, so the compiler would keep all of it in registers across this loop: past four rows the LDS
        // reads stay where they are written
        if constexpr (MT > 4) asm volatile("" ::: "memory");

        uint32_t acc[R * MT], cs[R];
        u32x4 x[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            x[r] = cur.b[r] ^ b_flip;
            cs[r] = 0u;
            if constexpr (CS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) cs[r] = dot4(x[r][j], kOnes, cs[r]);
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(&lds_a[(m * LK + c) * 4]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint32_t s = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) s = dot4(a[j], x[r][j], s);
                acc[r * MT + m] = s;
            }
        }

        lanes_reduce<R * MT, 1, kWave>(acc, c);
        uint32_t csv = 0u;
        if constexpr (CS) {
            lanes_reduce<R, 1, kWave>(cs, c);                      // lane r holds the column sum of row r of the iteration
            csv = static_cast<uint32_t>(__shfl(static_cast<int>(cs[0]), (c % (R * MT)) / MT, kWave));
        }
        if (c < R * MT) {
            const uint32_t m = c % MT, n = row0 + (c / MT) * RP + rp;
            if (m < p.M && n < p.N) emit<DQ>(p, split, m, n, acc[0], lds_rs[m], csv, ks, za, decode_col(p, n));
        }
        cur = nxt;
    }
}

// ---- the 8- and 16-row tiers of an NK matrix on the matrix cores
//
// 16 rows on dot4 are 16 instructions per dword of B, an LDS read of A per four of them and a butterfly of 70 shuffles per 16 rows of
// B: the tier is bound by instruction issue (docs/LAB_NOTES_r27.md).  v_mfma_i32_16x16x64_i8 takes the 16 rows as its A operand.  B
// still goes straight from global memory into registers in 16-byte loads; what changes is who multiplies.
//   wave      a tile of 16 rows of B (lane & 15) over the 1024 k of the slice: lane (c, qd = lane >> 4) loads the 16 bytes at
//             k = 64 s + 16 qd of span s -- that IS the operand image of the instruction ("Tile"), so B needs
//             neither LDS nor a shuffle and no butterfly follows.  The 16 loads of the next tile are issued before the MFMAs of this one.
//   A         [row][k] in LDS, rows padded by 16 bytes (16 lanes x 16 bytes: 16 different bank quads); rows >= M are zeros.
//   sums      the column sums of B: one more MFMA per span against a fragment of ones (every row of the result holds them).
//   route     taken where every 16-byte chunk of B is one aligned load inside K or lies past it: rows of B 16-byte aligned and K a
//             multiple of 16 (every model width).  Other operands keep the dot4 kernel above, whose guarded loads go byte by byte
//             -- 16 spans of those, twice, are more code than the register file holds.
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int kMmaRow = kQlDecodeSlice + 16;      // bytes of a row of A in LDS
constexpr int kMmaSpans = kQlDecodeSlice / 64;    // MFMA depths of a slice

// `lds_a`: kQlDecodeMaxRows * kMmaRow bytes, 16-byte aligned; `lds_rs`: kQlDecodeMaxRows dwords
template <bool CS, bool QA, bool DQ>
__device__ __forceinline__ void ql_decode_nk_mma_body(const QdArgs& p, unsigned char* const lds_a, uint32_t* const lds_rs) {
    constexpr int MT = kQlDecodeMaxRows, LK = kQlDecodeSlice / 16, WAVES = kQlDecodeThreads / kWave;
    constexpr int CH = chunks_per_thread(MT);
    static_assert(kQlDecodeColUnitNK == 16, "a workgroup's columns are whole tiles");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, qd = lane >> 4;
    const uint32_t split = blockIdx.x % p.splits, col_block = blockIdx.x / p.splits;
    const uint32_t k0 = split * kQlDecodeSlice;              // below K
    const u32x4 a_flip{p.a_flip, p.a_flip, p.a_flip, p.a_flip}, b_flip{p.b_flip, p.b_flip, p.b_flip, p.b_flip};
    {
        u32x4 v[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads, m = id / LK;
            v[i] = a_flip;
            if (m < static_cast<int>(p.M)) v[i] = stage_a16<QA>(p, m, k0 + 16 * (id % LK));
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads;
            *reinterpret_cast<u32x4*>(lds_a + (id / LK) * kMmaRow + 16 * (id % LK)) = v[i] ^ a_flip;
        }
    }
    __syncthreads();
    row_sums<MT, false, kMmaRow / 4>(p, reinterpret_cast<const uint32_t*>(lds_a), lds_rs, kQlDecodeSlice / 4, tid);

    const uint32_t za = shifted_a_zp(p);
    const uint32_t ks = min(p.K, k0 + kQlDecodeSlice) - k0;
    const uint32_t n_begin = col_block * p.cols_per_block, n_end = min(p.N, n_begin + p.cols_per_block);
    const unsigned char* const a_frag = lds_a + c * kMmaRow + 16 * qd;      // + 64 s: the lane's 16 bytes of span s
    const i32x4 ones{static_cast<int32_t>(kOnes), static_cast<int32_t>(kOnes), static_cast<int32_t>(kOnes), static_cast<int32_t>(kOnes)};

    struct Stage {
        u32x4 b[kMmaSpans];
    };
    auto load = [&](Stage& st, uint32_t n) {
#pragma unroll
        for (int s = 0; s < kMmaSpans; ++s) {
            st.b[s] = b_flip;
            const uint32_t k = k0 + 64 * s + 16 * qd;      // K is a multiple of 16 here: a chunk lies inside K or past it
            if (n < p.N && k < p.K) st.b[s] = *reinterpret_cast<const u32x4*>(p.B + static_cast<int64_t>(n) * p.ldb + k);
        }
    };

    Stage cur, nxt;
    load(cur, n_begin + wave * 16 + c);
    for (uint32_t t0 = n_begin + wave * 16; t0 < n_end; t0 += WAVES * 16) {      // the tile: rows t0 ... t0 + 15 of B
        nxt = cur;
        if (t0 + WAVES * 16 < n_end) load(nxt, t0 + WAVES * 16 + c);
        asm volatile("" ::: "memory");      // A's fragments are read where they are used, not kept in registers across the tiles

        i32x4 acc{0, 0, 0, 0}, cs{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < kMmaSpans; ++s) {
            if (k0 + 64 * s < p.K) {
                const i32x4 b = __builtin_bit_cast(i32x4, cur.b[s] ^ b_flip);
                const i32x4 a = *reinterpret_cast<const i32x4*>(a_frag + 64 * s);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
                if constexpr (CS) cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, cs, 0, 0, 0);
            }
        }

        // C/D map of the 16x16 MFMAs: column = lane & 15 (the row of B), row = 4 (lane >> 4) + r (the row of A)
        const uint32_t n = t0 + c;
        if (n < p.N) {
            const ColTerms col = decode_col(p, n);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m = 4 * qd + r;
                if (m < p.M) emit<DQ>(p, split, m, n, static_cast<uint32_t>(acc[r]), lds_rs[m], static_cast<uint32_t>(cs[r]), ks, za, col);
            }
        }
        cur = nxt;
    }
}

// dwords of the KN kernel's buffer: A's slice, and later the three other waves' values on their way to wave 0
constexpr int ql_decode_kn_lds_dwords(int mt, bool cs) {
    const int a = mt * (kQlDecodeSlice / 4), red = (kQlDecodeThreads / kWave - 1) * kWave * (mt * 4 + (cs ? 4 : 0));
    return a > red ? a : red;
}

// `lds`: ql_decode_kn_lds_dwords(MT, CS) dwords, 16-byte aligned; `lds_rs`: kQlDecodeMaxRows dwords
template <int MT, bool CS, bool QA, bool DQ>
__device__ __forceinline__ void ql_decode_kn_body(const QdArgs& p, uint32_t* const lds, uint32_t* const lds_rs) {
    constexpr int WAVES = kQlDecodeThreads / kWave;
    constexpr int VALS = MT * 4 + (CS ? 4 : 0);              // what a lane hands to wave 0
    constexpr int CH = chunks_per_thread(MT);
    static_assert(kQlDecodeColsKN == 4 * kWave && kQlDecodeSliceUnit == WAVES * 16, "a lane owns 4 columns, a wave's stage is 16 k");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t split = blockIdx.x % p.splits, col_block = blockIdx.x / p.splits;
    const uint32_t k0 = split * p.slice;                     // below K
    const int chunks = static_cast<int>(p.slice / 16);       // 16-byte chunks of a row of A's slice
    {
        u32x4 v[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads, m = id % MT, ch = id / MT;
            v[i] = u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
            if (ch < chunks && m < static_cast<int>(p.M)) v[i] = stage_a16<QA>(p, m, k0 + 16 * ch);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int id = tid + i * kQlDecodeThreads, m = id % MT, ch = id / MT;
            if (ch < chunks) {
#pragma unroll
                for (int j = 0; j < 4; ++j) lds[(4 * ch + j) * MT + m] = v[i][j] ^ p.a_flip;
            }
        }
    }
    __syncthreads();
    row_sums<MT, true>(p, lds, lds_rs, 4 * chunks, tid);

    const uint32_t n4 = col_block * kQlDecodeColsKN + 4 * lane;
    const uint32_t wave_k = p.slice / WAVES;                 // a multiple of 16
    const uint32_t kb = k0 + wave * wave_k;
    const int stages = static_cast<int>(wave_k / 16);
    const uint8_t* at = n4 < p.N ? p.B + static_cast<int64_t>(kb) * p.ldb + n4 : nullptr;      // row kb, column n4; moves on by 16 rows a stage

    struct Stage {
        uint32_t b[16];                                      // columns n4 ... + 3 of 16 consecutive k
    };
    auto load = [&](Stage& st, uint32_t k) {                 // called for kb, kb + 16, ... in this order
#pragma unroll
        for (int t = 0; t < 16; ++t) st.b[t] = (at && k + t < p.K) ? load_n4(at + t * p.ldb, n4, p.N, p.b_vec != 0) : p.b_flip;
        if (at) at += 16 * p.ldb;
    };

    uint32_t acc[MT * 4], cs[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) acc[i] = 0u;

    Stage cur, nxt;
    if (stages > 0) load(cur, kb);
    for (int s = 0; s < stages; ++s) {
        nxt = cur;
        if (s + 1 < stages) load(nxt, kb + 16 * (s + 1));
        const int q0 = static_cast<int>(wave * wave_k / 4) + 4 * s;       // the stage's first dword of A's rows
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // from 8 rows on the LDS reads of A stay with their dword of k: all 16 of a stage hoisted are 64 registers
            if constexpr (MT > 4) asm volatile("" ::: "memory");
            // r[j]: columns n4 .. + 3 at k + j  ->  cc[j]: k .. k + 3 of column n4 + j
            const uint32_t r0 = cur.b[4 * q] ^ p.b_flip, r1 = cur.b[4 * q + 1] ^ p.b_flip, r2 = cur.b[4 * q + 2] ^ p.b_flip, r3 = cur.b[4 * q + 3] ^ p.b_flip;
            const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
            const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
            const uint32_t cc[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                                    __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
            if constexpr (CS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) cs[j] = dot4(cc[j], kOnes, cs[j]);
            }
            if constexpr (MT == 1) {
                const uint32_t a = lds[q0 + q];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = dot4(a, cc[j], acc[j]);
            } else {
#pragma unroll
                for (int g = 0; g < MT / 4; ++g) {
                    const u32x4 a = *reinterpret_cast<const u32x4*>(&lds[(q0 + q) * MT + 4 * g]);
#pragma unroll
                    for (int mm = 0; mm < 4; ++mm)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[(4 * g + mm) * 4 + j] = dot4(a[mm], cc[j], acc[(4 * g + mm) * 4 + j]);
                }
            }
        }
        cur = nxt;
    }

    // the waves' quarters of the slice, added in wave order through the buffer that held A
    __syncthreads();
    if (wave > 0) {
        uint32_t* const mine = lds + (wave - 1) * kWave * VALS;
#pragma unroll
        for (int i = 0; i < MT * 4; ++i) mine[i * kWave + lane] = acc[i];
        if constexpr (CS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mine[(MT * 4 + j) * kWave + lane] = cs[j];
        }
    }
    __syncthreads();
    if (wave != 0 || n4 >= p.N) return;
#pragma unroll 1      // one wave's values at a time: all three in flight at once are 3 x VALS registers
    for (int w = 1; w < WAVES; ++w) {
        const uint32_t* const theirs = lds + (w - 1) * kWave * VALS;
#pragma unroll
        for (int i = 0; i < MT * 4; ++i) acc[i] += theirs[i * kWave + lane];
        if constexpr (CS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cs[j] += theirs[(MT * 4 + j) * kWave + lane];
        }
    }
    const uint32_t za = shifted_a_zp(p);
    const uint32_t ks = min(p.K, k0 + p.slice) - k0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t n = n4 + j;
        if (n >= p.N) break;
        const ColTerms c = decode_col(p, n);
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < static_cast<int>(p.M)) emit<DQ>(p, split, m, n, acc[m * 4 + j], lds_rs[m], cs[j], ks, za, c);
    }
}

// the slabs of a split K, added in slab order (uint32: any order gives the same bits), plus C, finished
template <bool DQ>
__device__ __forceinline__ void ql_decode_reduce_body(const QdArgs& p) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kQlDecodeThreads + threadIdx.x;
    const int64_t count = static_cast<int64_t>(p.M) * p.N;
    if (i >= count) return;
    uint32_t v = p.slab[i];
    for (uint32_t s = 1; s < p.splits; ++s) v += p.slab[s * count + i];
    const uint32_t n = static_cast<uint32_t>(i % p.N);
    if (p.C) v += static_cast<uint32_t>(p.C[n]);
    finish_acc<DQ>(p, static_cast<uint32_t>(i / p.N), n, static_cast<int32_t>(v), out_scale(p, n));
}

// ---- host
struct QdPlan : QlDecodePlan {      // and the workspace: include/oq_hip_qlinear_decode.h, `workspace`
    uint32_t* slab;
};

QdPlan make_plan(int64_t M, int64_t K, int64_t N, int32_t b_layout, Workspace& ws) {
    QdPlan pl{make_ql_decode_plan(M, K, N, b_layout)};
    pl.slab = ws.take<uint32_t>(pl.slab_bytes);
    return pl;
}

// the 8- and 16-row tiers of an NK matrix whose 16-byte chunks are whole aligned loads: the matrix cores
bool mma_route(const QdArgs& p, const QdPlan& pl, bool kn) { return !kn && pl.tier >= 8 && p.b_vec && p.K % 16 == 0; }

}  // namespace
}  // namespace oq
