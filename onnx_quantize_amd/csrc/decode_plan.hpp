// The launch plan of the decode route of MatMulNBits (matmul_nbits_decode.hip; include/oq_hip_nbits_decode.h restates it): host
// arithmetic only, in the style of tile_plan.hpp.  The tile GEMMs keep their own plan; nothing here is shared with them.  The row
// tiers and their switch are also those of the QLinearMatMul decode route (qlinear_decode_plan.hpp includes this file).
// No HIP: tests/c/qlinear_decode_plan_walk.cpp replays both plans under AddressSanitizer with plain g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace oq {

inline int64_t plan_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// accumulator rows per instantiation of a decode kernel: 1, 4, 8, 16 (M = 1 / 2-4 / 5-8 / 9-16)
inline int decode_tier(int64_t M) { return M <= 1 ? 1 : M <= 4 ? 4 : M <= 8 ? 8 : 16; }

// the row-tier switch of the kernels: f(std::integral_constant<int, MT>)
template <typename F>
void with_decode_tier(int tier, F&& f) {
    switch (tier) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// [splits, M, N] 4-byte partial sums, 0 for one split
inline size_t decode_slab_bytes(int64_t splits, int64_t M, int64_t N) { return splits > 1 ? static_cast<size_t>(splits) * M * N * 4 : 0; }

constexpr int kDecodeMaxRows = 16;       // M of the route: 1 ... 16
constexpr int kDecodeSlice = 1024;       // k of one workgroup: its slice of A lives in LDS as fp32, 16 rows x 1024 x 4 bytes = 64 KiB
constexpr int kDecodeRowUnit = 64;       // a workgroup's rows of B are a multiple of this: whole iterations of every vector-ALU
                                         // instantiation (rows of a pass x rows in flight <= 32) and one 16-row tile for each of the 4 waves
constexpr int kDecodeWorkgroups = 512;   // wanted: two per compute unit of the MI355X -- or one, where one is all that fits: the 8- and
                                         // 16-row tiers of an fp32 A (three bf16 pieces of its slice: 97 KiB of the 160 KiB of LDS)
constexpr int kDecodeThreads = 256;

struct DecodePlan {
    int tier;                   // decode_tier(M)
    int64_t splits;             // slices of K, kDecodeSlice each (the last one short): > 1: each writes a slab, a second launch adds them
    int64_t rows_per_block;     // rows of B (columns of Y) of one workgroup
    int64_t row_blocks;
    int64_t grid;               // row_blocks * splits workgroups (blockIdx.x = row_block * splits + split)
    size_t slab_bytes;          // decode_slab_bytes(splits, M, N)
};

inline DecodePlan make_decode_plan(int64_t M, int64_t K, int64_t N, bool a_is_fp32) {
    DecodePlan pl;
    pl.tier = decode_tier(M);
    pl.splits = plan_ceil_div(K, kDecodeSlice);
    const int64_t want = std::max<int64_t>(1, (a_is_fp32 && pl.tier >= 8 ? kDecodeWorkgroups / 2 : kDecodeWorkgroups) / pl.splits);
    pl.rows_per_block = plan_ceil_div(plan_ceil_div(N, want), kDecodeRowUnit) * kDecodeRowUnit;
    pl.row_blocks = plan_ceil_div(N, pl.rows_per_block);
    pl.grid = pl.row_blocks * pl.splits;
    pl.slab_bytes = decode_slab_bytes(pl.splits, M, N);
    return pl;
}

}  // namespace oq
