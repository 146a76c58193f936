// The layout of a caller-provided workspace, written once.  An entry point describes its workspace in ONE layout
// function that runs `take` piece by piece against a Workspace.  The `*_workspace_bytes` query runs it on a measuring Workspace (no
// base: pieces are only added up), the entry point on a carving one (base and byte count: every `take` returns the piece's pointer).
// The calls and their order are the same, so what the query returns is what the entry point consumes.
//
// Pieces are aligned to 256 bytes, the project's convention, or to a smaller power of two where a piece only needs its element's;
// a piece occupies a whole number of its alignment units, and a zero-byte piece takes no room and moves nothing.  A base of any
// alignment is handled by starting the layout at the first 256-byte boundary at or behind it; the total carries one whole unit for
// that step (the worst case is a byte less; the headers have always stated `+ 256`), whatever the base is, so a call is refused or
// accepted by its byte count alone.  An entry point that refuses a misaligned base itself declares so (`aligned_base`), and its
// total carries no pad.
//
// Precondition: the operands of every size are bounded by the entry point (extent_ok, count_ok, matrix_ok) before the layout
// runs, so the sums fit a size_t.  Where that is broken nothing wraps: the total saturates at SIZE_MAX and fits() is false.
//
// Host-only, no HIP: tests/c/workspace_walk.cpp replays the layouts of the library under AddressSanitizer with plain g++.
#pragma once

#include <cstddef>
#include <cstdint>

namespace oq {

class Workspace {
public:
    static constexpr size_t kAlign = 256;

    // bytes rounded up to a multiple of `align` (a power of two): the stride of equal pieces that lie in ONE take
    static size_t padded(size_t bytes, size_t align = kAlign) {
        const size_t b = add(bytes, align - 1);
        return b == SIZE_MAX ? b : b & ~(align - 1);
    }

    explicit Workspace(bool aligned_base = false) : Workspace(nullptr, 0, aligned_base) {}      // measure
    Workspace(void* base, size_t bytes, bool aligned_base = false)                               // carve
        : base_(static_cast<char*>(base)), bytes_(bytes), pad_(aligned_base ? 0 : kAlign) {
        if (base_) base_ += (kAlign - reinterpret_cast<uintptr_t>(base_) % kAlign) % kAlign;
        declared_ok_ = !aligned_base || base_ == base;           // a false declaration: nothing fits, total() still says what is needed
    }

    // The next piece.  Carving: its pointer, or null where it does not lie inside the workspace.  Measuring: null.
    template <typename T = char>
    T* take(size_t bytes, size_t align = kAlign) {
        if (bytes == 0) return nullptr;
        const size_t begin = padded(off_, align);
        off_ = add(begin, padded(bytes, align));
        return base_ && fits() ? reinterpret_cast<T*>(base_ + begin) : nullptr;
    }

    bool carving() const { return base_ != nullptr; }
    size_t total() const { return add(off_, pad_); }
    // carving: what a last piece of this alignment may still take behind pieces that end on it -- for a buffer that is a budget, used as
    // far as it goes (the T-slice slabs of the Hessian kernels)
    size_t left(size_t align = kAlign) const { return fits() && padded(off_, align) == off_ ? (bytes_ - total()) & ~(align - 1) : 0; }
    // every piece handed out so far lies inside [base, base + bytes); no pointer of a piece is used before this has been asked
    bool fits() const { return base_ != nullptr && declared_ok_ && total() != SIZE_MAX && total() <= bytes_; }

private:
    static size_t add(size_t a, size_t b) { return a > SIZE_MAX - b ? SIZE_MAX : a + b; }

    char* base_;      // carving: the first 256-byte boundary of the caller's workspace
    size_t bytes_;
    size_t pad_;      // what the total carries for the step from the caller's pointer to that boundary
    size_t off_ = 0;  // from base_ to the end of the last piece
    bool declared_ok_;
};

}  // namespace oq
