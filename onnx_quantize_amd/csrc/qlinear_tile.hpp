// The tile route of the 8-bit products as bodies, for qlinear_function.hip (include/oq_hip_qlinear_function.h): the text of the kernels
// of qlinear_gemm.hip, each as a __device__ __forceinline__ function that a kernel wraps (the kernel declares the LDS and calls the
// body), with one policy, EP (qlinear_epilogue.hpp):
//   kEpQuantized     the epilogue of qlinear_gemm.hip (finish_acc);
//   kEpDequantized   it ends in Y = (fp32(q) - fp32(y_zp)) * y_scale as fp32 instead of the 8-bit q (finish_acc<DQ>);
//   kEpQdqFunction   the epilogue of a QDQ function with quantized activations (finish_qdq; qdq_function.hip): the bias dequantized
//                    per column, the output Q -> DQ, and for a dynamic output one (min, max) of the workgroup's valid elements.
// qlinear_gemm.hip keeps its own text and does NOT include this file: wrapped around these bodies with the flag off, six of its seven
// kernels -- the twenty lines of ql_sum_rows_kernel included -- compile to another order of instructions and other register numbers
// (docs/LAB_NOTES_r32.md, section 1), and scripts/compare_kernel_asm.py holds that file to its text.  So the argument struct, the
// bodies and the workspace layout below are a copy, as qdq_matmul.hip's kernel is one of matmul_nbits.hip's; the guarded loads, the
// correction terms and the epilogue (qlinear_epilogue.hpp) and the plan (tile_plan.hpp) are the one shared text.  The policy marks
// the only places where the copy departs from the original.
// What the tile is and how it is staged: qlinear_gemm.hip.
#pragma once

#include "half_elem.hpp"
#include "qlinear_epilogue.hpp"
#include "tile_plan.hpp"
#include "workspace.hpp"

#include "../../include/oq_hip_qlinear.h"

namespace oq {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kRow = kBK + 16;    // bytes of a tile row in LDS (kBK: one MFMA depth): 16 lanes x 16 bytes land in 16 different bank quads
constexpr int kColSlices = 8;      // partial column sums of a KN matrix: slices of K

struct QlArgs {
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
    const int32_t* rowsum;         // NULL: its multiplier zb' is zero
    const int32_t* colsum;         // NULL: its multiplier za' is zero; [colsum_slices][colsum_stride] partial sums
    uint32_t colsum_slices, colsum_stride;
    uint32_t* slab;                // split K: [splits, M, N]
    uint32_t M, N, K, tiles_m, steps_per_split;      // extents are below 2^31: 32-bit indices, 64-bit only where an offset is formed
};

constexpr int ql_gemm_lds_bytes(int mt) { return (32 * mt + kBN) * kRow; }

// `lds`: ql_gemm_lds_bytes(MT) bytes, 16-byte aligned, declared by the kernel
template <int MT, int LAYOUT, int EP, class P>
__device__ __forceinline__ void ql_gemm_body(const P& p, unsigned char* const lds) {
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = (BM * 4 + kThreads - 1) / kThreads;      // 16-byte chunks of the A tile per thread
    unsigned char* const lds_b = lds + BM * kRow;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    // the row tiles of one column tile are neighbours in the tile order, and each XCD takes one contiguous range of it: a tile of B is
    // read into one L2, not into all eight (speed only)
    const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t m0 = (tile % p.tiles_m) * BM, n0 = (tile / p.tiles_m) * kBN;      // below 2^31 + a tile
    const uint32_t k_begin = blockIdx.y * p.steps_per_split * kBK;                                 // below K + 64 splits
    const uint32_t k_end = min(p.K, k_begin + p.steps_per_split * kBK);

    u32x4 a_regs[A_CHUNKS];
    u32x4 b_regs[2];
    // KN: this thread's two 4 x 4 byte blocks: columns 4 nb ... + 3 at k = 8 kb ... + 7
    const int kn_nb = tid & 31, kn_kb = tid >> 5;

    // the pointers this thread loads through are formed once; a step only adds to them
    const uint8_t* a_row[A_CHUNKS];      // the row of chunk i; NULL: a row >= M, or no chunk (the 32-row tile has 128)
    const uint8_t* b_row[2];             // NK: likewise; KN: [0] points at (k_begin + 8 kb, n) and moves on by 64 rows a step
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) {
        const int id = tid + i * kThreads;
        const uint32_t m = m0 + (id >> 2);
        a_row[i] = (id < BM * 4 && m < p.M) ? p.A + static_cast<int64_t>(m) * p.lda : nullptr;
    }
    const uint32_t kn_n = n0 + 4 * kn_nb;
    if constexpr (LAYOUT == OQ_QL_NK) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t n = n0 + ((tid + i * kThreads) >> 2);
            b_row[i] = n < p.N ? p.B + static_cast<int64_t>(n) * p.ldb : nullptr;
        }
    } else {
        b_row[0] = kn_n < p.N ? p.B + static_cast<int64_t>(k_begin + 8 * kn_kb) * p.ldb + kn_n : nullptr;
        b_row[1] = nullptr;
    }

    auto load_step = [&](uint32_t k) {      // called for k_begin, k_begin + 64, ... in this order
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            a_regs[i] = u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
            if (a_row[i]) a_regs[i] = load_k16(a_row[i], k + (tid & 3) * 16, p.K, p.a_vec != 0, p.a_flip);
        }
        if constexpr (LAYOUT == OQ_QL_NK) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                b_regs[i] = u32x4{p.b_flip, p.b_flip, p.b_flip, p.b_flip};
                if (b_row[i]) b_regs[i] = load_k16(b_row[i], k + (tid & 3) * 16, p.K, p.b_vec != 0, p.b_flip);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t kk = k + 8 * kn_kb + 4 * i + j;
                    b_regs[i][j] = (kk < p.K && b_row[0]) ? load_n4(b_row[0] + (4 * i + j) * p.ldb, kn_n, p.N, p.b_vec != 0) : p.b_flip;
                }
            if (b_row[0]) b_row[0] += kBK * p.ldb;
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            if (id < BM * 4) *reinterpret_cast<u32x4*>(lds + (id >> 2) * kRow + (id & 3) * 16) = a_regs[i] ^ u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
        }
        if constexpr (LAYOUT == OQ_QL_NK) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int id = tid + i * kThreads;
                *reinterpret_cast<u32x4*>(lds_b + (id >> 2) * kRow + (id & 3) * 16) = b_regs[i] ^ u32x4{p.b_flip, p.b_flip, p.b_flip, p.b_flip};
            }
        } else {
            uint32_t c[2][4];      // r[j]: columns n .. n + 3 at k + j  ->  c[j]: k .. k + 3 of column n + j
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t r0 = b_regs[i][0] ^ p.b_flip, r1 = b_regs[i][1] ^ p.b_flip, r2 = b_regs[i][2] ^ p.b_flip, r3 = b_regs[i][3] ^ p.b_flip;
                const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
                const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
                c[i][0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[i][1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
                c[i][2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[i][3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<u32x2*>(lds_b + (4 * kn_nb + ((j + (kn_nb >> 2)) & 3)) * kRow + 8 * kn_kb) = u32x2{c[0][j], c[1][j]};
        }
    };

    i32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = i32x4{0, 0, 0, 0};

    const unsigned char* const a_frag = lds + (wm * 16 * MT + (lane & 15)) * kRow + (lane >> 4) * 16;
    const unsigned char* b_frag[NT];      // KN: the column's rotated row (store_step)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int c16 = lane & 15, row = LAYOUT == OQ_QL_NK ? c16 : (c16 & 12) | ((c16 + nt) & 3);
        b_frag[nt] = lds_b + (wn * 64 + nt * 16 + row) * kRow + (lane >> 4) * 16;
    }

    if (k_begin < k_end) load_step(k_begin);
    for (uint32_t k = k_begin; k < k_end; k += kBK) {
        store_step();
        __syncthreads();
        if (k + kBK < k_end) load_step(k + kBK);
        i32x4 b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = *reinterpret_cast<const i32x4*>(b_frag[nt]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const i32x4 a = *reinterpret_cast<const i32x4*>(a_frag + mt * 16 * kRow);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 MFMAs: column = lane & 15, row = 4 (lane >> 4) + r
    const uint32_t col = n0 + wn * 64 + (lane & 15);
    [[maybe_unused]] MinMax mm;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const uint32_t n = col + 16 * nt;
        if (n >= p.N) continue;
        ColTerms c{};
        if (!p.slab) c = col_terms(p, n);
        [[maybe_unused]] float bias = 0.0f;
        if constexpr (EP == kEpQdqFunction)
            if (!p.slab) bias = qdq_bias(p, n);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m = m0 + wm * 16 * MT + mt * 16 + 4 * (lane >> 4) + r;
                if (m < p.M) {
                    const uint32_t S = static_cast<uint32_t>(acc[mt][nt][r]);
                    if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = S;
                    else if constexpr (EP == kEpQdqFunction) finish_qdq(p, m, n, S, c, bias, mm);
                    else finish<EP == kEpDequantized>(p, m, n, S, c);
                }
            }
    }
    if constexpr (EP == kEpQdqFunction)      // the k loop's last barrier is behind every read of the tiles: LDS is free
        if (!p.slab && p.out_mode == kQdqDynamic) block_minmax_store(mm, reinterpret_cast<float*>(lds), p.pairs, blockIdx.x);
}

// the slabs of a split K, added (uint32: any order gives the same bits), corrected and finished
// `red` (kEpQdqFunction only): 2 floats per wave of LDS, declared by the kernel
template <int EP, class P>
__device__ __forceinline__ void ql_reduce_body(const P& p, const int splits, [[maybe_unused]] float* red = nullptr) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int64_t count = static_cast<int64_t>(p.M) * p.N;
    if constexpr (EP == kEpQdqFunction) {      // every thread reaches the workgroup's fold
        MinMax mm;
        if (i < count) {
            uint32_t S = p.slab[i];
            for (int s = 1; s < splits; ++s) S += p.slab[s * count + i];
            const uint32_t n = static_cast<uint32_t>(i % p.N);
            finish_qdq(p, static_cast<uint32_t>(i / p.N), n, S, col_terms(p, n), qdq_bias(p, n), mm);
        }
        if (p.out_mode == kQdqDynamic) block_minmax_store(mm, red, p.pairs, blockIdx.x);
    } else {
        if (i >= count) return;
        uint32_t S = p.slab[i];
        for (int s = 1; s < splits; ++s) S += p.slab[s * count + i];
        const uint32_t n = static_cast<uint32_t>(i % p.N);
        finish<EP == kEpDequantized>(p, static_cast<uint32_t>(i / p.N), n, S, col_terms(p, n));
    }
}

__device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

// sums[r] = sum_k x'[r, k] of a [rows, K] matrix whose fast axis is k (A; B in NK): one wave per row.  x' = (x ^ ubias) - 128 as an
// unsigned byte, ubias = 0x80 for a signed operand: v_sad_u8 adds the four bytes of a dword in one instruction.
__device__ __forceinline__ void ql_sum_rows_body(const uint8_t* X, int64_t rows, int64_t K, int64_t ld, uint32_t ubias, int32_t vec, int32_t* sums) {
    const int lane = threadIdx.x & 63;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint8_t* x = X + row * ld;
    uint32_t s = 0u;
    int64_t done = 0;
    if (vec) {                                  // rows are 4-byte aligned
        const int64_t K4 = K / 4;
        for (int64_t i = lane; i < K4; i += kWave) s = __builtin_amdgcn_sad_u8(reinterpret_cast<const uint32_t*>(x)[i] ^ ubias, 0u, s);
        done = K4 * 4;
    }
    for (int64_t k = done + lane; k < K; k += kWave) s += (static_cast<uint32_t>(x[k]) ^ ubias) & 0xFFu;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s), off, 64));
    if (lane == 0) sums[row] = static_cast<int32_t>(s - 128u * static_cast<uint32_t>(K));
}

// sums[y][n] = sum of x'[k, n] over slice y of K, of a [K, N] matrix whose fast axis is n (B in KN): a block takes 64 columns of
// one slice, as 16 dwords x 16 phases of k.  `part`: LDS declared by the kernel
__device__ __forceinline__ void ql_sum_cols_body(const uint8_t* X, int64_t K, int64_t N, int64_t ld, uint32_t ubias, int32_t vec, int32_t* sums,
                                                 int64_t stride, uint32_t (*part)[64]) {
    const int cg = threadIdx.x & 15, ph = threadIdx.x >> 4;
    const int64_t n = static_cast<int64_t>(blockIdx.x) * 64 + 4 * cg;
    uint32_t s[4] = {0u, 0u, 0u, 0u};
    const int64_t per_slice = ceil_div_dev(K, gridDim.y), k_begin = min(K, blockIdx.y * per_slice), k_end = min(K, k_begin + per_slice);
    if (n < N)
        for (int64_t k = k_begin + ph; k < k_end; k += 16) {
            const uint32_t w = load_n4(X + k * ld + n, static_cast<uint32_t>(n), static_cast<uint32_t>(N), vec != 0) ^ ubias;
#pragma unroll
            for (int b = 0; b < 4; ++b) s[b] += (w >> (8 * b)) & 0xFFu;
        }
#pragma unroll
    for (int b = 0; b < 4; ++b) part[ph][4 * cg + b] = s[b];
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t total = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) total += part[i][threadIdx.x];
        const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
        if (c < N) sums[blockIdx.y * stride + c] = static_cast<int32_t>(total - 128u * static_cast<uint32_t>(k_end - k_begin));
    }
}

// ---- host
struct Plan : TilePlan {      // and the workspace: include/oq_hip_qlinear.h, `workspace`
    int32_t* rowsum;          // [M] sums of A's rows
    int32_t* colsum;          // [kColSlices] partial sums of B's columns, `colsum_stride` entries apart
    uint32_t colsum_stride;
    uint32_t* slab;
};

Plan make_plan(int64_t M, int64_t K, int64_t N, Workspace& ws) {
    Plan pl{make_tile_plan(M, K, N)};
    const size_t slice_bytes = Workspace::padded(static_cast<size_t>(N) * 4);
    pl.rowsum = ws.take<int32_t>(static_cast<size_t>(M) * 4);
    pl.colsum = ws.take<int32_t>(kColSlices * slice_bytes);
    pl.colsum_stride = static_cast<uint32_t>(slice_bytes / 4);
    pl.slab = ws.take<uint32_t>(pl.slab_bytes);
    return pl;
}


}  // namespace
}  // namespace oq
