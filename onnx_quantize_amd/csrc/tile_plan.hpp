// The block tiles and the split of K that the two fused GEMMs share (matmul_nbits.hip, qlinear_gemm.hip): host arithmetic only.
// Their kernels are each file's own -- they index in different widths on purpose (docs/LAB_NOTES_r24.md section 2).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace oq {

constexpr int kBN = 128;        // columns of a block tile
constexpr int kBK = 64;         // k of a step
constexpr int kThreads = 256;

struct TilePlan {
    int bm;                     // rows of a block tile: 32 (one MFMA row tile per wave, MT = 1) or 128 (MT = 4)
    int64_t tiles_m, tiles;     // block tiles along M, and in all (blockIdx.x)
    int64_t steps_per_split;    // kBK-deep steps of one block
    int64_t splits;             // blocks along K (blockIdx.y); > 1: each writes a slab of partial sums, a second launch adds them
    size_t slab_bytes;          // [splits, M, N] 4-byte partial sums, 0 for one split
};

// Few tiles leave most of the 256 compute units idle: K is split until about 256 blocks exist, 8 ways at the most.
inline TilePlan make_tile_plan(int64_t M, int64_t K, int64_t N) {
    const auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    TilePlan pl;
    pl.bm = M <= 32 ? 32 : 128;
    pl.tiles_m = ceil_div(M, pl.bm);
    pl.tiles = pl.tiles_m * ceil_div(N, kBN);
    const int64_t steps = ceil_div(K, kBK);
    const int64_t want = pl.tiles >= 128 ? 1 : std::min<int64_t>(std::min<int64_t>(8, steps), 256 / pl.tiles);
    pl.steps_per_split = ceil_div(steps, want);
    pl.splits = ceil_div(steps, pl.steps_per_split);
    pl.slab_bytes = pl.splits > 1 ? static_cast<size_t>(pl.splits) * M * N * 4 : 0;
    return pl;
}

// the MT = 1 / 4 switch of both kernels: f(std::integral_constant<int, MT>)
template <typename F>
void with_row_tiles(const TilePlan& pl, F&& f) {
    if (pl.bm == 32) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 4>{});
}

}  // namespace oq
