// The launch plan of the decode route of an 8-bit QDQ function with quantized activations (qdq_function_decode.hip;
// include/oq_hip_qdq_function_decode.h restates it): host arithmetic only, in the style of qdq_function_packed4_decode_plan.hpp, whose
// numbers it keeps -- the A slice in LDS and the slabs cost here what they cost there.  The tile route keeps its own plan.
#pragma once

#include "decode_plan.hpp"

namespace oq {

constexpr int kQfDecodeMaxRows = 16;        // M of the route: 1 ... 16, the rows of one matrix instruction
constexpr int kQfDecodeCols = 128;          // a workgroup's columns: 16 column slots of a wave x 8 bytes: one 128-byte line of a row
constexpr int kQfDecodeSpan = 64;           // the k of one matrix instruction; a slice is a multiple of it, a wave's quarter of 16
constexpr int kQfDecodeMaxSlice = 2048;     // the longest slice of K: X's slice lies in LDS as bytes, 16 rows x (2048 + pad) = 33 KiB
// wanted workgroups: two per compute unit of the MI355X for M <= 4; above, one -- the quantizing of a slice of X is repeated by every
// column block and the slabs grow with the number of slices.
constexpr int kQfDecodeWorkgroups = 512;

struct QfDecodePlan {
    int64_t slice;          // k of one workgroup
    int64_t splits;         // slices of K (the last one short): > 1: each writes a slab, a second launch adds them
    int64_t col_blocks;     // grid: (col_blocks, splits)
    size_t slab_bytes;      // decode_slab_bytes(splits, M, N), int32 partial sums
    int64_t x_blocks;       // workgroups of the min / max pass over a dynamic X: one wave per row
    int64_t out_blocks;     // workgroups that finish Y, each leaving one (min, max) pair for a dynamic output
};

inline QfDecodePlan make_qf_decode_plan(int64_t M, int64_t K, int64_t N) {
    QfDecodePlan pl;
    pl.col_blocks = plan_ceil_div(N, kQfDecodeCols);
    const int64_t want = plan_ceil_div(M <= 4 ? kQfDecodeWorkgroups : kQfDecodeWorkgroups / 2, pl.col_blocks);
    pl.slice = std::min<int64_t>(kQfDecodeMaxSlice, plan_ceil_div(plan_ceil_div(K, want), kQfDecodeSpan) * kQfDecodeSpan);
    pl.splits = plan_ceil_div(K, pl.slice);
    pl.slab_bytes = decode_slab_bytes(pl.splits, M, N);
    pl.x_blocks = plan_ceil_div(M, 4);
    pl.out_blocks = pl.splits == 1 ? pl.col_blocks : plan_ceil_div(M * N, 256);
    return pl;
}

}  // namespace oq
