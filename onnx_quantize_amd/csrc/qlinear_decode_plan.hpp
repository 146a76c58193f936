// The launch plan of the decode route of QLinearMatMul / QGemm (qlinear_decode.hip; include/oq_hip_qlinear_decode.h restates it):
// host arithmetic only.  The row tiers, their switch and the slab size are those of decode_plan.hpp; the slice and block rules are
// this route's own.  The tile GEMM keeps its own plan; nothing here is shared with it.
// No HIP: tests/c/qlinear_decode_plan_walk.cpp replays it under AddressSanitizer with plain g++.
#pragma once

#include "decode_plan.hpp"

namespace oq {

constexpr int kQlDecodeMaxRows = 16;        // M of the route: 1 ... 16
constexpr int kQlDecodeThreads = 256;
constexpr int kQlDecodeLayoutKN = 0, kQlDecodeLayoutNK = 1;      // oq_ql_layout
constexpr int kQlDecodeSlice = 1024;        // the longest slice of K: A's slice lies in LDS as bytes, 16 rows x 1024 = 16 KiB.  NK: every
                                            // slice is this long (64 lanes x 16 bytes: a wave spans it)
constexpr int kQlDecodeSliceUnit = 64;      // KN: a slice is a multiple of this -- 4 waves x one stage of 16 k
constexpr int kQlDecodeColUnitNK = 16;      // NK: a workgroup's columns (rows of B) are a multiple of 4 waves x 4 rows in flight
constexpr int kQlDecodeColsKN = 256;        // KN: a workgroup's columns: 64 lanes x 4 columns, whatever N is
constexpr int kQlDecodeWorkgroups = 512;    // wanted: two per compute unit of the MI355X; the 8- and 16-row tiers of a KN matrix want one
                                            // (a slice more is M * N * 8 bytes of slab traffic, and only K slices fill the device there)

struct QlDecodePlan {
    int tier;                   // decode_tier(M)
    int64_t slice;              // k of one workgroup
    int64_t splits;             // slices of K (the last one short): > 1: each writes a slab, a second launch adds them
    int64_t cols_per_block;     // columns of Y of one workgroup
    int64_t col_blocks;
    int64_t grid;               // col_blocks * splits workgroups (blockIdx.x = col_block * splits + split)
    size_t slab_bytes;          // decode_slab_bytes(splits, M, N), int32 partial sums
};

inline QlDecodePlan make_ql_decode_plan(int64_t M, int64_t K, int64_t N, int layout) {
    QlDecodePlan pl;
    pl.tier = decode_tier(M);
    if (layout == kQlDecodeLayoutNK) {
        pl.slice = kQlDecodeSlice;
        pl.splits = plan_ceil_div(K, pl.slice);
        const int64_t want = std::max<int64_t>(1, kQlDecodeWorkgroups / pl.splits);
        pl.cols_per_block = plan_ceil_div(plan_ceil_div(N, want), kQlDecodeColUnitNK) * kQlDecodeColUnitNK;
    } else {
        pl.cols_per_block = kQlDecodeColsKN;
        const int64_t want = plan_ceil_div(pl.tier >= 8 ? kQlDecodeWorkgroups / 2 : kQlDecodeWorkgroups, plan_ceil_div(N, pl.cols_per_block));
        pl.slice = std::min<int64_t>(kQlDecodeSlice, plan_ceil_div(plan_ceil_div(K, want), kQlDecodeSliceUnit) * kQlDecodeSliceUnit);
        pl.splits = plan_ceil_div(K, pl.slice);
    }
    pl.col_blocks = plan_ceil_div(N, pl.cols_per_block);
    pl.grid = pl.col_blocks * pl.splits;
    pl.slab_bytes = decode_slab_bytes(pl.splits, M, N);
    return pl;
}

}  // namespace oq
