// Host-side guard for the workspace carver (csrc/workspace.hpp), built by tests/test_workspace_guard.py with
// g++ -fsanitize=address,undefined.  It replays layouts of the library -- the pieces an entry point takes, as plain lists of
// (bytes, align) -- against heap blocks of EXACTLY the measured size, at every alignment of the base: a measuring run that promised
// less than the carving run hands out is a heap-buffer-overflow here, where on the device it would be a write into someone else's
// memory.  One byte fewer must be refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "workspace.hpp"

using oq::Workspace;

struct Piece {
    size_t bytes, align;
};
struct Layout {
    const char* name;
    bool aligned_base;      // the entry point refuses a base that is not 256-byte aligned (oq_matmul_nbits, oq_qlinear_matmul)
    std::vector<Piece> pieces;
};

// the calls of a layout function: the same ones, in the same order, whether `ws` measures or carves
static std::vector<unsigned char*> run(const Layout& l, Workspace& ws) {
    std::vector<unsigned char*> p;
    for (const Piece& k : l.pieces) p.push_back(ws.take<unsigned char>(k.bytes, k.align));
    return p;
}

static int bad = 0;
static void expect(bool ok, const Layout& l, const char* what, size_t at) {
    if (ok) return;
    printf("FAILED %s: %s (%zu)\n", l.name, what, at);
    ++bad;
}

// carves [base, base + bytes), writes the first and the last byte of every piece (ASan: outside the block -> abort), then checks
// alignment, order and bounds of what was handed out
static void carve_and_touch(const Layout& l, unsigned char* base, size_t bytes) {
    Workspace ws(base, bytes, l.aligned_base);
    const std::vector<unsigned char*> p = run(l, ws);
    expect(ws.fits(), l, "the measured size does not fit", bytes);
    if (!ws.fits()) return;
    unsigned char* end_of_last = base;
    for (size_t i = 0; i < p.size(); ++i) {
        const Piece& k = l.pieces[i];
        if (k.bytes == 0) {
            expect(p[i] == nullptr, l, "a zero-byte piece got a pointer", i);
            continue;
        }
        p[i][0] = static_cast<unsigned char>(i + 1);
        p[i][k.bytes - 1] = static_cast<unsigned char>(i + 1);
        expect(reinterpret_cast<uintptr_t>(p[i]) % k.align == 0, l, "piece misaligned", i);
        expect(p[i] >= end_of_last, l, "piece overlaps the one before", i);
        expect(p[i] + k.bytes <= base + bytes, l, "piece leaves the workspace", i);
        end_of_last = p[i] + k.bytes;
    }
    for (size_t i = 0; i < p.size(); ++i)      // nobody wrote over a neighbour's ends
        if (l.pieces[i].bytes != 0)
            expect(p[i][0] == static_cast<unsigned char>(i + 1) && p[i][l.pieces[i].bytes - 1] == static_cast<unsigned char>(i + 1), l, "piece overwritten", i);
}

static void refuse(const Layout& l, unsigned char* base, size_t bytes, const char* what) {
    Workspace ws(base, bytes, l.aligned_base);
    run(l, ws);
    expect(!ws.fits(), l, what, bytes);
}

static void walk(const Layout& l) {
    Workspace measure(l.aligned_base);
    for (unsigned char* p : run(l, measure)) expect(p == nullptr, l, "a measuring run handed out a pointer", 0);
    expect(!measure.fits(), l, "a measuring run fits", 0);
    const size_t need = measure.total();
    if (l.aligned_base) {
        if (need == 0) return;      // nothing to carve: such a call takes no workspace at all
        void* block = nullptr;
        if (posix_memalign(&block, 256, need) != 0) abort();
        unsigned char* base = static_cast<unsigned char*>(block);
        carve_and_touch(l, base, need);
        refuse(l, base, need - 1, "one byte fewer fits");
        refuse(l, base + 8, need - 8, "a misaligned base was taken");
        free(block);
        return;
    }
    for (size_t shift = 0; shift < 256; ++shift) {      // malloc aligns to 16: every residue of the base modulo 256 occurs
        unsigned char* block = static_cast<unsigned char*>(malloc(need + shift));
        carve_and_touch(l, block + shift, need);
        refuse(l, block + shift, need - 1, "one byte fewer fits");
        free(block);
    }
}

int main() {
    const size_t A = Workspace::kAlign;
    std::vector<Layout> layouts = {
        // oq_gptq_loop_f32, K = 256, N = 64 (gptq_loop.hip: loop_layout): Err, carried scale / zp, the per-group parameters, the working
        // copy of a tall block, coefficient images, the two operands' pieces, the MSE search's workspace
        {"gptq_loop block 128", false, {{65536, A}, {256, A}, {256, A}, {32768, A}, {8192, A}, {0, A}, {2 * 5000, A}, {147456, A}, {81920, A}, {84262, A}}},
        {"gptq_loop block 256 (tall)", false, {{65536, A}, {256, A}, {256, A}, {32768, A}, {8192, A}, {65536, A}, {2 * 5000, A}, {147456, A}, {81920, A}, {84262, A}}},
        {"gptq_loop odd N = 37", false, {{37888, A}, {148, A}, {148, A}, {18944, A}, {4736, A}, {0, A}, {5000, A}, {147456, A}, {81920, A}, {82900, A}}},
        // oq_hqq_optimize (hqq.hip: hqq_layout), K = 128, N = 64, g = 64: rows = 128, parts = 2; control words, partials, zero points
        {"hqq one pass", false, {{64, 64}, {2 * 8 * 32, 8}, {128 * 4 * 33, 4}}},
        {"hqq per round", false, {{64, 64}, {2 * 8, 8}, {128 * 4, 4}, {128 * 4, 4}, {128 * 4, 4}}},
        {"hqq per round, odd rows", false, {{64, 64}, {3 * 8, 8}, {37 * 4, 4}, {37 * 4, 4}, {37 * 4, 4}}},
        // the MSE search (rtn_mse.hip: mse_layout), K = 256, N = 64: the head (stop word, tensor range), rows of 12 bytes, tensor partials
        {"rtn_mse group 128", false, {{256, A}, {128 * 12, 4}, {1024 * 20 * 4, 4}}},
        {"rtn_mse tensor", false, {{256, A}, {12, 4}, {1024 * 20 * 4, 4}}},
        {"rtn_mse 37 rows", false, {{256, A}, {37 * 12, 4}, {1024 * 20 * 4, 4}}},
        // oq_matmul_nbits (matmul_nbits.hip: make_plan), M = 16, K = 512, N = 128: fp32 A -> two pieces and the row exponents; 8 splits
        {"matmul_nbits fp32 A, split K", true, {{16 * 512 * 2, A}, {16 * 512 * 2, A}, {16 * 4, A}, {8 * 16 * 128 * 4, A}}},
        {"matmul_nbits fp16 A, split K", true, {{0, A}, {0, A}, {0, A}, {8 * 16 * 128 * 4, A}}},
        {"matmul_nbits fp16 A, one split", true, {{0, A}, {0, A}, {0, A}, {0, A}}},
        {"matmul_nbits fp32 A, M = 3, K = 100", true, {{3 * 104 * 2, A}, {3 * 104 * 2, A}, {3 * 4, A}, {2 * 3 * 7 * 4, A}}},
        // oq_qlinear_matmul (qlinear_gemm.hip: make_plan), the same shape: row sums, eight slices of column sums, the slabs
        {"qlinear_matmul split K", true, {{16 * 4, A}, {8 * 512, A}, {8 * 16 * 128 * 4, A}}},
        {"qlinear_matmul M = 3, N = 7", true, {{3 * 4, A}, {8 * 256, A}, {2 * 3 * 7 * 4, A}}},
        // oq_gptq_factor_f32, K = 192 (factor.hip: factor_layout): P, Lt, X, Y, the inverted diagonal blocks, no piece inverse
        {"gptq_factor K = 192", false, {{147456, A}, {147456, A}, {147456, A}, {147456, A}, {131072, A}, {0, A}}},
        // oq_abs_stats_cols_many_h16 (abs_stats_half.hip: stat_layout): one array of floats
        {"abs_stats two items", false, {{2 * 72 * 2 * 4, 8}}},
        // mixed alignments in an order that needs padding between the pieces
        {"mixed", false, {{1, 1}, {3, 2}, {5, 4}, {7, 8}, {1, 16}, {9, 64}, {1, A}, {2, 1}, {255, A}, {257, A}}},
        {"nothing", false, {}},
    };
    for (const Layout& l : layouts) walk(l);

    // sizes beyond a size_t saturate: nothing wraps to a small total that would fit
    {
        const Layout huge{"overflow", false, {{SIZE_MAX / 2, A}, {SIZE_MAX / 2, A}, {4096, A}}};
        Workspace measure;
        run(huge, measure);
        expect(measure.total() == SIZE_MAX, huge, "the total wrapped", measure.total());
        unsigned char block[4096];
        Workspace ws(block, sizeof(block));
        for (unsigned char* p : run(huge, ws)) expect(p == nullptr, huge, "a piece of a wrapped layout got a pointer", 0);
        expect(!ws.fits(), huge, "a wrapped layout fits", 0);
    }
    printf("layouts=%zu bad=%d\n", layouts.size(), bad);
    return bad ? 1 : 0;
}
