// Host-side walk of the launch plan of the QLinearMatMul / QGemm decode route (csrc/qlinear_decode_plan.hpp), built by
// tests/test_qlinear_decode_abi.py with g++ -fsanitize=address,undefined.  For every (M, K, N, layout) of a sweep that includes the
// model widths it replays who takes what, the way the kernels index: every k of [0, K) lies in exactly one slice (KN: in exactly one
// wave's stage of it), every column of [0, N) in exactly one workgroup's range, and the slab the entry point carves -- the same
// carver on a heap block of exactly the measured size -- is the measured one.  A count kept outside its array is an ASan abort.
// The MatMulNBits decode route (csrc/decode_plan.hpp, which the header above includes for the row tiers both routes share) is walked
// the same way: every k of [0, K) in exactly one slice, every row of B in exactly one workgroup's range and one iteration of it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qlinear_decode_plan.hpp"
#include "workspace.hpp"

using namespace oq;

static int bad = 0;
static void expect(bool ok, const char* what, int64_t M, int64_t K, int64_t N, int layout) {
    if (ok) return;
    printf("FAILED M=%lld K=%lld N=%lld layout=%d: %s\n", (long long)M, (long long)K, (long long)N, layout, what);
    ++bad;
}

static void walk(int64_t M, int64_t K, int64_t N, int layout) {
    const QlDecodePlan pl = make_ql_decode_plan(M, K, N, layout);
    auto check = [&](bool ok, const char* what) { expect(ok, what, M, K, N, layout); };
    check(pl.tier >= M && (pl.tier == 1 || pl.tier == 4 || pl.tier == 8 || pl.tier == 16), "the tier does not hold M rows");
    check(pl.slice > 0 && pl.slice <= kQlDecodeSlice && pl.slice % kQlDecodeSliceUnit == 0, "the slice is no multiple of its unit within A's LDS image");
    check(pl.grid == pl.col_blocks * pl.splits && pl.grid > 0 && pl.grid < (int64_t(1) << 31), "the grid");

    // k: slices, and for KN the four waves' stages of 16 k inside a slice
    std::vector<unsigned char> k_seen(static_cast<size_t>(K), 0);
    for (int64_t split = 0; split < pl.splits; ++split) {
        const int64_t k0 = split * pl.slice;
        check(k0 < K, "an empty slice");
        if (layout == kQlDecodeLayoutNK) {
            for (int lane = 0; lane < 64; ++lane)
                for (int b = 0; b < 16; ++b)
                    if (k0 + 16 * lane + b < K) ++k_seen[static_cast<size_t>(k0 + 16 * lane + b)];
        } else {
            const int64_t wave_k = pl.slice / 4, stages = wave_k / 16;
            check(stages * 16 * 4 == pl.slice, "the waves' stages do not tile the slice");
            for (int wave = 0; wave < 4; ++wave)
                for (int64_t s = 0; s < stages; ++s)
                    for (int t = 0; t < 16; ++t)
                        if (k0 + wave * wave_k + 16 * s + t < K) ++k_seen[static_cast<size_t>(k0 + wave * wave_k + 16 * s + t)];
        }
    }
    bool once = true;
    for (unsigned char c : k_seen) once = once && c == 1;
    check(once, "a k is covered not exactly once");

    // columns: NK iterations of 16 rows of B inside [n_begin, n_end); KN 64 lanes x 4 columns
    std::vector<unsigned char> n_seen(static_cast<size_t>(N), 0);
    for (int64_t cb = 0; cb < pl.col_blocks; ++cb) {
        const int64_t n_begin = cb * pl.cols_per_block, n_end = std::min(N, n_begin + pl.cols_per_block);
        check(n_begin < N, "an empty column block");
        if (layout == kQlDecodeLayoutNK) {
            check(pl.cols_per_block % kQlDecodeColUnitNK == 0, "a workgroup's columns are no whole iterations");
            for (int64_t row0 = n_begin; row0 < n_end; row0 += 16)
                for (int i = 0; i < 16; ++i)
                    if (row0 + i < N) ++n_seen[static_cast<size_t>(row0 + i)];
        } else {
            check(pl.cols_per_block == kQlDecodeColsKN, "a KN workgroup has 256 columns");
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    if (n_begin + 4 * lane + j < N) ++n_seen[static_cast<size_t>(n_begin + 4 * lane + j)];
        }
    }
    once = true;
    for (unsigned char c : n_seen) once = once && c == 1;
    check(once, "a column is covered not exactly once");

    // the slab: measured, then carved from a heap block of exactly that size and touched at both ends
    check(pl.slab_bytes == (pl.splits > 1 ? static_cast<size_t>(pl.splits) * M * N * 4 : 0), "the slab bytes");
    Workspace measure(/* aligned_base */ true);
    measure.take<uint32_t>(pl.slab_bytes);
    const size_t total = measure.total();
    check(total == Workspace::padded(pl.slab_bytes), "the measured size is not the padded slab");
    if (total == 0) return;
    unsigned char* block = static_cast<unsigned char*>(aligned_alloc(256, total));
    Workspace carve(block, total, /* aligned_base */ true);
    unsigned char* slab = reinterpret_cast<unsigned char*>(carve.take<uint32_t>(pl.slab_bytes));
    check(carve.fits() && slab == block, "the carved slab is not the measured one");
    if (carve.fits()) {
        // the last element a workgroup writes: slab (splits - 1), row M - 1, column N - 1
        const size_t last = ((static_cast<size_t>(pl.splits - 1) * M + (M - 1)) * N + (N - 1)) * 4;
        slab[0] = 1, slab[last + 3] = 1;
        check(last + 4 == pl.slab_bytes, "the last element is not the slab's last");
    }
    Workspace shorter(block, total - 1, /* aligned_base */ true);
    shorter.take<uint32_t>(pl.slab_bytes);
    check(!shorter.fits(), "one byte fewer was accepted");
    free(block);
}

static void walk_nbits(int64_t M, int64_t K, int64_t N, bool a_is_fp32) {
    const DecodePlan pl = make_decode_plan(M, K, N, a_is_fp32);
    auto check = [&](bool ok, const char* what) { expect(ok, what, M, K, N, a_is_fp32 ? -32 : -16); };
    check(pl.tier == decode_tier(M) && pl.tier >= M && pl.tier <= kDecodeMaxRows, "the tier does not hold M rows");
    int switched = 0;
    with_decode_tier(pl.tier, [&](auto mt) { switched = decltype(mt)::value; });
    check(switched == pl.tier, "the tier switch instantiates another tier");
    check(pl.grid == pl.row_blocks * pl.splits && pl.grid > 0 && pl.grid < (int64_t(1) << 31), "the grid");
    check(pl.slab_bytes == (pl.splits > 1 ? static_cast<size_t>(pl.splits) * M * N * 4 : 0), "the slab bytes");

    // k: a slice is LK lanes x VAL consecutive k -- 32 x 32 at 4 bits, 64 x 16 at 8
    std::vector<unsigned char> k_seen(static_cast<size_t>(K), 0);
    for (int64_t split = 0; split < pl.splits; ++split) {
        const int64_t k0 = split * kDecodeSlice;
        check(k0 < K, "an empty slice");
        for (int lane = 0; lane < 64; ++lane)
            for (int v = 0; v < 16; ++v)
                if (k0 + 16 * lane + v < K) ++k_seen[static_cast<size_t>(k0 + 16 * lane + v)];
    }
    bool once = true;
    for (unsigned char c : k_seen) once = once && c == 1;
    check(once, "a k is covered not exactly once");

    // rows of B: iterations of 8, 16 or 32 rows (vector ALU: rows of a pass x rows in flight) or 64 (matrix cores: 4 waves x 16)
    check(pl.rows_per_block % kDecodeRowUnit == 0, "a workgroup's rows are no whole iterations");
    for (int64_t step : {8, 16, 32, 64}) {
        std::vector<unsigned char> n_seen(static_cast<size_t>(N), 0);
        for (int64_t rb = 0; rb < pl.row_blocks; ++rb) {
            const int64_t n_begin = rb * pl.rows_per_block, n_end = std::min(N, n_begin + pl.rows_per_block);
            check(n_begin < N, "an empty row block");
            for (int64_t row0 = n_begin; row0 < n_end; row0 += step)
                for (int64_t i = 0; i < step; ++i)
                    if (row0 + i < N) ++n_seen[static_cast<size_t>(row0 + i)];
        }
        once = true;
        for (unsigned char c : n_seen) once = once && c == 1;
        check(once, "a row of B is covered not exactly once");
    }
}

int main() {
    const int64_t Ms[] = {1, 2, 4, 5, 8, 9, 16};
    const int64_t Ks[] = {1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2050, 4096, 11008};
    const int64_t Ns[] = {1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000, 4096, 11008, 32000};
    int walked = 0;
    for (int64_t M : Ms)
        for (int64_t K : Ks)
            for (int64_t N : Ns)
                for (int layout : {kQlDecodeLayoutKN, kQlDecodeLayoutNK}) walk(M, K, N, layout), ++walked;
    // the model widths land on one to two workgroups per compute unit (256 of them)
    for (int layout : {kQlDecodeLayoutKN, kQlDecodeLayoutNK})
        for (int64_t M : {int64_t(1), int64_t(16)}) {
            const int64_t shapes[][2] = {{4096, 11008}, {11008, 4096}, {4096, 4096}};
            for (const auto& s : shapes) {
                const QlDecodePlan pl = make_ql_decode_plan(M, s[0], s[1], layout);
                expect(pl.grid >= 192 && pl.grid <= 640, "a model width off one to two workgroups per compute unit", M, s[0], s[1], layout);
            }
        }
    int nbits_walked = 0;
    for (int64_t M : {int64_t(1), int64_t(4), int64_t(5), int64_t(16)})
        for (int64_t K : Ks)
            for (int64_t N : Ns)
                for (bool a_is_fp32 : {false, true}) walk_nbits(M, K, N, a_is_fp32), ++nbits_walked;
    printf("walked=%d nbits_walked=%d bad=%d\n", walked, nbits_walked, bad);
    return bad != 0;
}
