// The decode route of QLinearMatMul / com.microsoft::QGemm / MatMulInteger (include/oq_hip_qlinear_decode.h): M = 1 ... 16
// rows of A against an 8-bit B that is streamed ONCE from global memory straight into registers and never passes through LDS.
//
//       acc[m, n] = sum_k (A[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])       exact, int32 (two's-complement wrap)
//       Y[m, n]   = epilogue(acc[m, n])                                          qlinear_epilogue.hpp: the text qlinear_gemm.hip runs
//
// The products are signed dot4 (v_dot4_i32_i8 family: four bytes of A against four bytes of B a lane and instruction).  As in the
// tile kernel an unsigned operand is flipped on its way into the arithmetic (x ^ 0x80 per byte) and its zero point moves by 128; with
// a', za', b', zb' the flipped operands and shifted zero points, a slice s of K contributes
//
//       S_s - zb'[n] rowsum_s(a')[m] - za' colsum_s(b')[n] + K_s za' zb'[n]            (uint32: a wrap is defined)
//
//   block     256 threads; a slice of K (blockIdx.x % splits) and cols_per_block columns of Y (qlinear_decode_plan.hpp).
//   A         the slice of all M rows is staged once per workgroup into LDS as flipped bytes; rows >= M and k >= K are zeros of the
//             flipped operand.  Its row sums over the slice are taken from that image (one more dot4 against 0x01010101 per dword).
//   B         loaded as it lies in memory; the flip is applied where a register is consumed, an iteration after its load was issued.
//             Past K a guarded load delivers the flip's byte (a zero after the flip); columns >= N are never stored.  The column sums
//             come from the registers that feed the product: one more dot4 against 0x01010101 per dword.
//   NK        B[n, k]: lane c of a wave owns the 16 bytes at k = 16 c of the 1024-k slice, the 4 waves take different rows, 4 rows
//             are in flight per lane (16 rows an iteration), those of the next iteration are issued before the arithmetic of this
//             one.  A lies [row][k]: a lane reads its 16 bytes of each row (consecutive lanes, consecutive 16 bytes).  The 4 x MT sums
//             and the 4 column sums of a lane are added over the 64 lanes by the transposing butterfly (lanes_reduce.hpp).
//   KN        B[k, n]: a lane owns 4 columns -- a wave's 64 lanes cover 256 consecutive bytes of a row -- and walks k: 16 rows a
//             stage, the next stage issued before the arithmetic of this one; each 4 x 4 byte block is transposed in registers
//             (v_perm_b32) into four dwords, k ... k + 3 of one column each.  A lies [k / 4][row]: its dwords are wave-uniform, one
//             LDS read serves four rows.  The 4 waves take quarters of the slice and are added through LDS in wave order (the
//             buffer is A's: it is dead by then); wave 0 corrects and finishes.
//   sums      a sum whose multiplier is zero on the host's knowledge (the other operand signed, its zero-point pointer NULL) is skipped.
//   split K   splits > 1: the corrected partial value goes to int32 slab `split`; ql_decode_reduce_kernel adds the slabs in slab
//             order, adds C and finishes.  No atomics, no workgroup waits on another, nothing synchronises with the host.
// The 8- and 16-row tiers of an NK matrix whose rows are 16-byte aligned (K a multiple of 16) run ql_decode_nk_mma_kernel (further down)
// instead: the same streaming, the products on the matrix cores.
// Shared: the guarded loads, the epilogue, the checks of a call and the operand block with qlinear_gemm.hip (qlinear_epilogue.hpp); the
// row tiers and the butterfly with matmul_nbits_decode.hip (decode_plan.hpp, lanes_reduce.hpp).
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
__device__ __forceinline__ void emit(const QdArgs& p, uint32_t split, uint32_t m, uint32_t n, uint32_t S, uint32_t rs, uint32_t cs, uint32_t ks,
                                     uint32_t za, const ColTerms& c) {
    const uint32_t v = S - c.zb * rs - za * cs + ks * za * c.zb;
    if (p.slab) p.slab[(static_cast<int64_t>(split) * p.M + m) * p.N + n] = v;
    else finish_acc(p, m, n, static_cast<int32_t>(v + c.add), c.scale);
}

constexpr int chunks_per_thread(int mt) { return (mt * (kQlDecodeSlice / 16) + kQlDecodeThreads - 1) / kQlDecodeThreads; }

template <int MT, bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void ql_decode_nk_kernel(const QdArgs p) {
    constexpr int R = 4;                                     // rows of B in flight per lane
    constexpr int RP = kQlDecodeThreads / kWave;             // rows of a pass: one per wave
    constexpr int LK = kQlDecodeSlice / 16;                  // lanes along k: a wave
    constexpr int CH = chunks_per_thread(MT);
    static_assert(LK == kWave && R * MT <= kWave && RP * R == kQlDecodeColUnitNK, "the transposing reduce leaves value c in lane c");
    __shared__ __attribute__((aligned(16))) uint32_t lds_a[MT * (kQlDecodeSlice / 4)];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];

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
            if (id < MT * LK && m < static_cast<int>(p.M)) v[i] = load_k16(p.A + static_cast<int64_t>(m) * p.lda, k0 + 16 * (id % LK), p.K, p.a_vec != 0, p.a_flip);
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
            if (m < p.M && n < p.N) emit(p, split, m, n, acc[0], lds_rs[m], csv, ks, za, decode_col(p, n));
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

template <bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void ql_decode_nk_mma_kernel(const QdArgs p) {
    constexpr int MT = kQlDecodeMaxRows, LK = kQlDecodeSlice / 16, WAVES = kQlDecodeThreads / kWave;
    constexpr int CH = chunks_per_thread(MT);
    static_assert(kQlDecodeColUnitNK == 16, "a workgroup's columns are whole tiles");
    __shared__ __attribute__((aligned(16))) unsigned char lds_a[MT * kMmaRow];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];

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
            if (m < static_cast<int>(p.M)) v[i] = load_k16(p.A + static_cast<int64_t>(m) * p.lda, k0 + 16 * (id % LK), p.K, p.a_vec != 0, p.a_flip);
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
                if (m < p.M) emit(p, split, m, n, static_cast<uint32_t>(acc[r]), lds_rs[m], static_cast<uint32_t>(cs[r]), ks, za, col);
            }
        }
        cur = nxt;
    }
}

template <int MT, bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void ql_decode_kn_kernel(const QdArgs p) {
    constexpr int WAVES = kQlDecodeThreads / kWave;
    constexpr int VALS = MT * 4 + (CS ? 4 : 0);              // what a lane hands to wave 0
    constexpr int A_DWORDS = MT * (kQlDecodeSlice / 4), RED_DWORDS = (WAVES - 1) * kWave * VALS;
    constexpr int CH = chunks_per_thread(MT);
    static_assert(kQlDecodeColsKN == 4 * kWave && kQlDecodeSliceUnit == WAVES * 16, "a lane owns 4 columns, a wave's stage is 16 k");
    __shared__ __attribute__((aligned(16))) uint32_t lds[A_DWORDS > RED_DWORDS ? A_DWORDS : RED_DWORDS];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];

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
            if (ch < chunks && m < static_cast<int>(p.M)) v[i] = load_k16(p.A + static_cast<int64_t>(m) * p.lda, k0 + 16 * ch, p.K, p.a_vec != 0, p.a_flip);
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
            if (m < static_cast<int>(p.M)) emit(p, split, m, n, acc[m * 4 + j], lds_rs[m], cs[j], ks, za, c);
    }
}

// the slabs of a split K, added in slab order (uint32: any order gives the same bits), plus C, finished
__global__ __launch_bounds__(kQlDecodeThreads) void ql_decode_reduce_kernel(const QdArgs p) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kQlDecodeThreads + threadIdx.x;
    const int64_t count = static_cast<int64_t>(p.M) * p.N;
    if (i >= count) return;
    uint32_t v = p.slab[i];
    for (uint32_t s = 1; s < p.splits; ++s) v += p.slab[s * count + i];
    const uint32_t n = static_cast<uint32_t>(i % p.N);
    if (p.C) v += static_cast<uint32_t>(p.C[n]);
    finish_acc(p, static_cast<uint32_t>(i / p.N), n, static_cast<int32_t>(v), out_scale(p, n));
}

// ---- host
struct Plan : QlDecodePlan {      // and the workspace: include/oq_hip_qlinear_decode.h, `workspace`
    uint32_t* slab;
};

Plan make_plan(int64_t M, int64_t K, int64_t N, int32_t b_layout, Workspace& ws) {
    Plan pl{make_ql_decode_plan(M, K, N, b_layout)};
    pl.slab = ws.take<uint32_t>(pl.slab_bytes);
    return pl;
}

// the 8- and 16-row tiers of an NK matrix whose 16-byte chunks are whole aligned loads: the matrix cores
bool mma_route(const QdArgs& p, const Plan& pl, bool kn) { return !kn && pl.tier >= 8 && p.b_vec && p.K % 16 == 0; }

template <bool CS>
void launch(const QdArgs& p, const Plan& pl, bool kn, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(pl.grid);
    if (mma_route(p, pl, kn)) {
        ql_decode_nk_mma_kernel<CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
        return;
    }
    with_decode_tier(pl.tier, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        if (kn) ql_decode_kn_kernel<MT, CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
        else ql_decode_nk_kernel<MT, CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
    });
}

}  // namespace
}  // namespace oq

using namespace oq;

static_assert(kQlDecodeLayoutKN == OQ_QL_KN && kQlDecodeLayoutNK == OQ_QL_NK, "the plan header's layout codes are the ABI's");

extern "C" {

int32_t oq_qlinear_decode_extension_version(void) { return OQ_QLINEAR_DECODE_EXTENSION_VERSION; }

size_t oq_qlinear_matmul_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t b_layout) {
    if (!shape_ok(M, K, N) || M > kQlDecodeMaxRows || !layout_ok(b_layout)) {
        set_error("oq_qlinear_matmul_decode_workspace_bytes: M=%lld K=%lld N=%lld b_layout=%d outside the bounds of the decode route", (long long)M,
                  (long long)K, (long long)N, b_layout);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, b_layout, ws);
    return ws.total();
}

int32_t oq_qlinear_matmul_decode(const void* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale, const void* a_zero_point,
                                 const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale,
                                 const void* b_zero_point, int32_t b_per_column, const int32_t* C, const float* y_scale, const void* y_zero_point,
                                 int32_t flags, int32_t out, void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qlinear_matmul_decode";
    int32_t st = call_ok(fn, kQlDecodeMaxRows, A, a_type, M, K, lda, a_scale, B, b_type, b_layout, N, ldb, b_scale, C, y_scale, flags, out, Y, ldy);
    if (st != OQ_OK) return st;
    const bool kn = b_layout == OQ_QL_KN;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, b_layout, ws);
    OQ_REQUIRE(ws.total() == 0 || ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    QdArgs p{};
    fill_operands(p, A, a_type, M, K, lda, a_scale, a_zero_point, B, b_type, b_layout, N, ldb, b_scale, b_zero_point, b_per_column, C, y_scale,
                  y_zero_point, out, Y, ldy);
    p.slice = static_cast<uint32_t>(pl.slice), p.splits = static_cast<uint32_t>(pl.splits), p.cols_per_block = static_cast<uint32_t>(pl.cols_per_block);
    p.slab = pl.slab;
    p.need_rowsum = sum_needed(p.b_signed, b_zero_point);
    if (sum_needed(p.a_signed, a_zero_point)) launch<true>(p, pl, kn, s);
    else launch<false>(p, pl, kn, s);
    st = check_launch(kn ? "ql_decode_kn_kernel" : "ql_decode_nk_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    ql_decode_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kQlDecodeThreads)), kQlDecodeThreads, 0, s>>>(p);
    return check_launch("ql_decode_reduce_kernel");
}

}  // extern "C"
