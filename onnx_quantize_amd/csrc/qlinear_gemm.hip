// QLinearMatMul / com.microsoft::QGemm / MatMulInteger on the int8 matrix cores (include/oq_hip_qlinear.h):
//
//       acc[m, n] = sum_k (A[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])       exact, int32 (two's-complement wrap)
//       Y[m, n]   = epilogue(acc[m, n])
//
// v_mfma_i32_16x16x64_i8 is signed x signed: an unsigned operand is flipped while it is staged (x ^ 0x80 per byte, one VALU op per
// dword) and its zero point moves by 128.  With a' = a - 128 [A unsigned], za' = a_zp - 128 [A unsigned], and b', zb' likewise:
//
//       acc = S - zb'[n] rowsum_k(a')[m] - za' colsum_k(b')[n] + K za' zb'[n],           S = sum_k a' b' from the MFMAs.
//
//   block     256 threads = 2 x 2 waves; tile 32 * MT rows (MT = 4: 128; MT = 1: 32, for M <= 32) x 128 columns; k-step 64 = one
//             MFMA depth.  Tiling, plan and split K are those of matmul_nbits.hip.
//   operands  both tiles lie in LDS with k as the fast axis, 64 bytes a row, padded to 80: lane l reads 16 bytes of row / column
//             l & 15 at byte 16 (l >> 4) -- 16 different bank quads.  Which k of the 64 the instruction takes from which byte does
//             not matter: A and B are read from the same image, so byte j of lane group g meets byte j of lane group g.
//   A, B (NK) staged directly: 16-byte global loads along k (byte loads where rows are not 16-byte aligned, or at K's end).
//   B (KN)    the fast axis in memory is n: a thread loads 8 dwords -- 4 columns of 8 consecutive k -- with the 32 lanes of a half
//             wave on the 128 consecutive bytes of one k, transposes the two 4 x 4 byte blocks in registers (v_perm_b32) and writes
//             4 x 8 bytes, each 8 consecutive k of one column, into the [n][k] image.  Columns of equal n mod 4 share a bank quad,
//             so column 4 q + j lies in row 4 q + (j + (q >> 2)) mod 4: the half wave's writes land in 16 bank quads, two lanes
//             each, and the 16 columns of a fragment read still cover 16.  Rows that are not 4-byte aligned take byte loads.
//   staging   registers: the global loads of step i + 1 are issued before the MFMAs of step i; one LDS buffer, two barriers a step.
//   guards    rows >= M and k >= K are zeros in LDS AFTER the flip (a pad of 0 is 0 of the flipped operand): the flip is applied on
//             the way into LDS, and a padded position is staged as the flip's own byte.  Columns >= N are computed on whatever the
//             guarded loads gave and never stored.
//   sums      ql_sum_rows_kernel / ql_sum_cols_kernel write rowsum(a') and colsum(b') into the workspace.  The column sums of a KN
//             matrix are written as 8 partial sums over eighths of K (blocks enough to fill the device on a [4096, 4096] weight,
//             no second pass and no atomics); whoever reads a column sum adds the 8.
//   split K   blockIdx.y takes a range of k-steps and writes S to int32 slab y; ql_reduce_kernel adds the slabs, corrects and
//             finishes.  No atomics anywhere.
// The guarded loads, the epilogue, the checks of a call and the operand block of the argument struct are those of the decode route
// too: qlinear_epilogue.hpp.
#include "half_elem.hpp"
#include "qlinear_epilogue.hpp"
#include "tile_plan.hpp"

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

template <int MT, int LAYOUT>
__global__ __launch_bounds__(kThreads, 2) void ql_gemm_kernel(const QlArgs p) {
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = (BM * 4 + kThreads - 1) / kThreads;      // 16-byte chunks of the A tile per thread
    __shared__ __attribute__((aligned(16))) unsigned char lds[(BM + kBN) * kRow];
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
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const uint32_t n = col + 16 * nt;
        if (n >= p.N) continue;
        ColTerms c{};
        if (!p.slab) c = col_terms(p, n);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m = m0 + wm * 16 * MT + mt * 16 + 4 * (lane >> 4) + r;
                if (m < p.M) {
                    const uint32_t S = static_cast<uint32_t>(acc[mt][nt][r]);
                    if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = S;
                    else finish(p, m, n, S, c);
                }
            }
    }
}

// the slabs of a split K, added (uint32: any order gives the same bits), corrected and finished
__global__ __launch_bounds__(kThreads) void ql_reduce_kernel(const QlArgs p, const int splits) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int64_t count = static_cast<int64_t>(p.M) * p.N;
    if (i >= count) return;
    uint32_t S = p.slab[i];
    for (int s = 1; s < splits; ++s) S += p.slab[s * count + i];
    const uint32_t n = static_cast<uint32_t>(i % p.N);
    finish(p, static_cast<uint32_t>(i / p.N), n, S, col_terms(p, n));
}

__device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

// sums[r] = sum_k x'[r, k] of a [rows, K] matrix whose fast axis is k (A; B in NK): one wave per row.  x' = (x ^ ubias) - 128 as an
// unsigned byte, ubias = 0x80 for a signed operand: v_sad_u8 adds the four bytes of a dword in one instruction.
__global__ __launch_bounds__(kThreads) void ql_sum_rows_kernel(const uint8_t* X, int64_t rows, int64_t K, int64_t ld, uint32_t ubias, int32_t vec,
                                                               int32_t* sums) {
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
// one slice, as 16 dwords x 16 phases of k
__global__ __launch_bounds__(kThreads) void ql_sum_cols_kernel(const uint8_t* X, int64_t K, int64_t N, int64_t ld, uint32_t ubias, int32_t vec,
                                                               int32_t* sums, int64_t stride) {
    __shared__ uint32_t part[16][64];
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

template <int LAYOUT>
void launch_gemm(const QlArgs& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { ql_gemm_kernel<decltype(mt)::value, LAYOUT><<<grid, kThreads, 0, s>>>(p); });
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qlinear_extension_version(void) { return OQ_QLINEAR_EXTENSION_VERSION; }

size_t oq_qlinear_matmul_workspace_bytes(int64_t M, int64_t K, int64_t N) {
    if (!shape_ok(M, K, N)) {
        set_error("oq_qlinear_matmul_workspace_bytes: M=%lld K=%lld N=%lld outside the bounds", (long long)M, (long long)K, (long long)N);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, ws);
    return ws.total();
}

int32_t oq_qlinear_matmul(const void* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale, const void* a_zero_point,
                          const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point,
                          int32_t b_per_column, const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags, int32_t out, void* Y,
                          int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qlinear_matmul";
    int32_t st = call_ok(fn, kMaxExtent, A, a_type, M, K, lda, a_scale, B, b_type, b_layout, N, ldb, b_scale, C, y_scale, flags, out, Y, ldy);
    if (st != OQ_OK) return st;
    const bool kn = b_layout == OQ_QL_KN;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    QlArgs p{};
    fill_operands(p, A, a_type, M, K, lda, a_scale, a_zero_point, B, b_type, b_layout, N, ldb, b_scale, b_zero_point, b_per_column, C, y_scale,
                  y_zero_point, out, Y, ldy);
    p.tiles_m = static_cast<uint32_t>(pl.tiles_m), p.steps_per_split = static_cast<uint32_t>(pl.steps_per_split);
    int32_t* rowsum = sum_needed(p.b_signed, b_zero_point) ? pl.rowsum : nullptr;
    int32_t* colsum = sum_needed(p.a_signed, a_zero_point) ? pl.colsum : nullptr;
    p.rowsum = rowsum, p.colsum = colsum;
    p.colsum_slices = kn ? kColSlices : 1, p.colsum_stride = pl.colsum_stride;
    p.slab = pl.slab;

    // the sums run over x ^ ubias read as an unsigned byte, minus 128: ubias flips a SIGNED operand
    const uint32_t a_ubias = p.a_flip ^ 0x80808080u, b_ubias = p.b_flip ^ 0x80808080u;
    constexpr int kRowsPerBlock = kThreads / kWave;
    if (rowsum) {
        ql_sum_rows_kernel<<<static_cast<unsigned>(ceil_div(M, kRowsPerBlock)), kThreads, 0, s>>>(p.A, M, K, lda, a_ubias,
                                                                                                  aligned_to(A, 4) && lda % 4 == 0, rowsum);
        st = check_launch("ql_sum_rows_kernel");
        if (st != OQ_OK) return st;
    }
    if (colsum) {
        const int32_t vec4 = aligned_to(B, 4) && ldb % 4 == 0;
        if (kn) ql_sum_cols_kernel<<<dim3(static_cast<unsigned>(ceil_div(N, 64)), kColSlices), kThreads, 0, s>>>(p.B, K, N, ldb, b_ubias, vec4, colsum, p.colsum_stride);
        else ql_sum_rows_kernel<<<static_cast<unsigned>(ceil_div(N, kRowsPerBlock)), kThreads, 0, s>>>(p.B, N, K, ldb, b_ubias, vec4, colsum);
        st = check_launch(kn ? "ql_sum_cols_kernel" : "ql_sum_rows_kernel");
        if (st != OQ_OK) return st;
    }
    if (kn) launch_gemm<OQ_QL_KN>(p, pl, s);
    else launch_gemm<OQ_QL_NK>(p, pl, s);
    st = check_launch("ql_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    ql_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kThreads)), kThreads, 0, s>>>(p, static_cast<int>(pl.splits));
    return check_launch("ql_reduce_kernel");
}

}  // extern "C"
