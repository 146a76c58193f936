// What the tile GEMMs on the exact (q - zp) matrix-core operand share (matmul_nbits.hip: B is the MatMulNBits blob; qdq_matmul.hip:
// W is a [K, N] byte matrix): the argument block, the one rounding of a sum to Y's type, the guarded load
// of eight elements of A, the kernel that adds the slabs of a split K, the kernel that splits an fp32 A into two fp16 pieces, and
// the plan with its workspace.  Each file's GEMM kernel is its own: they differ in how B reaches LDS and in nothing else.
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

}  // namespace
}  // namespace oq
