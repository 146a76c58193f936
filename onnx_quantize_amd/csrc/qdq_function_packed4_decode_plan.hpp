// The launch plan of the decode route of a W4A8 QDQ function (qdq_function_packed4_decode.hip;
// include/oq_hip_qdq_function_packed4_decode.h restates it): host arithmetic only, in the style of qlinear_decode_plan.hpp.  The tile
// route keeps its own plan; nothing here is shared with it.
#pragma once

#include "decode_plan.hpp"

namespace oq {

constexpr int kP4DecodeMaxRows = 16;        // M of the route: 1 ... 16, the rows of one matrix instruction
constexpr int kP4DecodeCols = 128;          // a workgroup's columns: 16 column slots of a wave x one dword of 8 nibbles
constexpr int kP4DecodeSpan = 64;           // the k of one matrix instruction; a slice is a multiple of it, a wave's quarter of 16
constexpr int kP4DecodeMaxSlice = 2048;     // the longest slice of K: X's slice lies in LDS as bytes, 16 rows x (2048 + pad) = 33 KiB
// wanted workgroups: two per compute unit of the MI355X for M <= 4.  Above, a workgroup's quantizing of its slice of X (M * slice
// divisions, repeated by every column block) and the slabs (splits * M * N * 4 bytes next to K * N / 2 of W) both grow with the
// number of slices: one per compute unit.
constexpr int kP4DecodeWorkgroups = 512;

struct P4DecodePlan {
    int64_t slice;          // k of one workgroup
    int64_t splits;         // slices of K (the last one short): > 1: each writes a slab, a second launch adds them
    int64_t col_blocks;     // grid: (col_blocks, splits)
    size_t slab_bytes;      // decode_slab_bytes(splits, M, N), int32 partial sums
    int64_t x_blocks;       // workgroups of the min / max pass over a dynamic X: one wave per row
    int64_t out_blocks;     // workgroups that finish Y, each leaving one (min, max) pair for a dynamic output
};

inline P4DecodePlan make_p4_decode_plan(int64_t M, int64_t K, int64_t N) {
    P4DecodePlan pl;
    pl.col_blocks = plan_ceil_div(N, kP4DecodeCols);
    const int64_t want = plan_ceil_div(M <= 4 ? kP4DecodeWorkgroups : kP4DecodeWorkgroups / 2, pl.col_blocks);
    pl.slice = std::min<int64_t>(kP4DecodeMaxSlice, plan_ceil_div(plan_ceil_div(K, want), kP4DecodeSpan) * kP4DecodeSpan);
    pl.splits = plan_ceil_div(K, pl.slice);
    pl.slab_bytes = decode_slab_bytes(pl.splits, M, N);
    pl.x_blocks = plan_ceil_div(M, 4);
    pl.out_blocks = pl.splits == 1 ? pl.col_blocks : plan_ceil_div(M * N, 256);
    return pl;
}

}  // namespace oq
