// Host-side walk of the workspace of oq_qdq_function (include/oq_hip_qdq_function.h, `workspace`; csrc/qdq_function.hip:
// make_qdq_function_plan), built by tests/test_qdq_function_abi.py with g++ -fsanitize=address,undefined as a stand-alone program.
// The pieces Q, R, C, S, P, PX, PO are taken -- with the library's own plan (csrc/tile_plan.hpp) and carver (csrc/workspace.hpp) --
// from a heap block of EXACTLY the size the header's formula gives: a formula that promised less than the carver hands out is a
// heap-buffer-overflow here.  One byte fewer and a misaligned base must be refused.  Prints one line per shape for the test to
// compare with the library's query.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tile_plan.hpp"
#include "workspace.hpp"

using oq::Workspace;

enum { NONE = 0, STATIC = 1, DYNAMIC = 2 };

static size_t r256(size_t n) { return Workspace::padded(n); }
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Piece {
    const char* name;
    size_t bytes;
};

// the takes of make_qdq_function_plan, in its order
static std::vector<Piece> pieces(int64_t M, int64_t K, int64_t N, int x_mode, int out_mode) {
    const oq::TilePlan pl = oq::make_tile_plan(M, K, N);
    const size_t out_blocks = pl.splits == 1 ? pl.tiles : ceil_div(M * N, 256);
    return {{"Q", static_cast<size_t>(M * ceil_div(K, 16) * 16)},
            {"R", static_cast<size_t>(M) * 4},
            {"C", 8 * r256(static_cast<size_t>(N) * 4)},
            {"S", pl.slab_bytes},
            {"P", x_mode == DYNAMIC ? size_t(12) : 0},
            {"PX", x_mode == DYNAMIC ? static_cast<size_t>(std::min<int64_t>(ceil_div(M, 4), 2048)) * 8 : 0},
            {"PO", out_mode == DYNAMIC ? out_blocks * 8 : 0}};
}

// the header's formula, term by term
static size_t formula(int64_t M, int64_t K, int64_t N, int x_mode, int out_mode) {
    const oq::TilePlan pl = oq::make_tile_plan(M, K, N);
    size_t total = r256(M * ceil_div(K, 16) * 16) + r256(M * 4) + 8 * r256(N * 4) + (pl.splits > 1 ? r256(pl.splits * M * N * 4) : 0);
    if (x_mode == DYNAMIC) total += 256 + r256(8 * std::min<int64_t>(ceil_div(M, 4), 2048));
    if (out_mode == DYNAMIC) total += r256(8 * (pl.splits == 1 ? pl.tiles : ceil_div(M * N, 256)));
    return total;
}

static int bad = 0;
static void expect(bool ok, const char* what, int64_t M, int64_t K, int64_t N, int x_mode, int out_mode) {
    if (ok) return;
    printf("FAILED M=%lld K=%lld N=%lld x_mode=%d out_mode=%d: %s\n", (long long)M, (long long)K, (long long)N, x_mode, out_mode, what);
    ++bad;
}

static void walk(int64_t M, int64_t K, int64_t N, int x_mode, int out_mode) {
    const std::vector<Piece> ps = pieces(M, K, N, x_mode, out_mode);
    Workspace measure(/* aligned_base */ true);
    for (const Piece& p : ps) expect(measure.take<unsigned char>(p.bytes) == nullptr, "a measuring run handed out a pointer", M, K, N, x_mode, out_mode);
    const size_t need = formula(M, K, N, x_mode, out_mode);
    expect(measure.total() == need, "the carver's total is not the header's formula", M, K, N, x_mode, out_mode);
    printf("%lld %lld %lld %d %d %zu\n", (long long)M, (long long)K, (long long)N, x_mode, out_mode, need);

    void* block = nullptr;
    if (posix_memalign(&block, 256, need) != 0) abort();
    unsigned char* const base = static_cast<unsigned char*>(block);
    Workspace ws(base, need, true);
    std::vector<unsigned char*> got;
    for (const Piece& p : ps) got.push_back(ws.take<unsigned char>(p.bytes));
    expect(ws.fits(), "the formula's size does not fit", M, K, N, x_mode, out_mode);
    if (ws.fits()) {
        unsigned char* end_of_last = base;
        for (size_t i = 0; i < ps.size(); ++i) {
            if (ps[i].bytes == 0) {
                expect(got[i] == nullptr, "a zero-byte piece got a pointer", M, K, N, x_mode, out_mode);
                continue;
            }
            got[i][0] = got[i][ps[i].bytes - 1] = static_cast<unsigned char>(i + 1);      // ASan: outside the block -> abort
            expect(reinterpret_cast<uintptr_t>(got[i]) % 256 == 0, "piece misaligned", M, K, N, x_mode, out_mode);
            expect(got[i] >= end_of_last && got[i] + ps[i].bytes <= base + need, "piece overlaps or leaves the workspace", M, K, N, x_mode, out_mode);
            end_of_last = got[i] + ps[i].bytes;
        }
        for (size_t i = 0; i < ps.size(); ++i)
            if (ps[i].bytes != 0)
                expect(got[i][0] == i + 1 && got[i][ps[i].bytes - 1] == i + 1, "piece overwritten", M, K, N, x_mode, out_mode);
    }
    for (const size_t shift : {size_t(0), size_t(8)}) {      // one byte fewer; a misaligned base
        Workspace less(base + shift, need - (shift ? shift : 1), true);
        for (const Piece& p : ps) less.take<unsigned char>(p.bytes);
        expect(!less.fits(), shift ? "a misaligned base was taken" : "one byte fewer fits", M, K, N, x_mode, out_mode);
    }
    free(block);
}

int main() {
    const int64_t shapes[][3] = {{1, 1, 1}, {16, 63, 100}, {33, 65, 100}, {129, 200, 260}, {1, 1088, 1}, {16, 1088, 260}, {129, 1088, 130},
                                 {64, 1024, 1024}, {2048, 4096, 11008}, {16, 11008, 4096}, {9000, 64, 130}};
    int walked = 0;
    for (const auto& s : shapes)
        for (int x_mode : {STATIC, DYNAMIC})
            for (int out_mode : {NONE, STATIC, DYNAMIC}) walk(s[0], s[1], s[2], x_mode, out_mode), ++walked;
    printf("walked=%d bad=%d\n", walked, bad);
    return bad ? 1 : 0;
}
