// The element types of the operands W and X -- fp32, fp16, bf16 -- and everything that depends on which of them a call carries:
// the exact conversion to fp32 at the load, the ABI's type code of an element type, the dispatcher from a type code to an element
// type, and the host check every _h16 entry point makes of its 2-byte operand.  A kernel that reads W or X is a
// template on one of these structs and nothing else.  Users: awq.hip, rtn_mse.hip, hqq.hip (all three types); rtn_half.hip,
// reduce_half.hip, abs_stats_half.hip (the 2-byte types); gemm_tn.hip (the check, and the type code of its piece kernels).
#pragma once

#include <cstdint>
#include <type_traits>

#include "oq_common.hpp"

#include "../../include/oq_hip_half.h"

namespace oq {

// `raw` is what memory holds; one(raw) is its value as fp32, two(word) the values of the two elements of a 32-bit word (the 2-byte
// types only, low half first).  Every conversion is exact.
struct ElemF32 {
    typedef float raw;
    static __device__ __forceinline__ float one(float b) { return b; }
};
struct ElemF16 {
    typedef uint16_t raw;
    static __device__ __forceinline__ float one(uint16_t b) { return static_cast<float>(__builtin_bit_cast(_Float16, b)); }
    static __device__ __forceinline__ void two(uint32_t w, float& lo, float& hi) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 v = __builtin_bit_cast(h2, w);
        lo = static_cast<float>(v[0]);
        hi = static_cast<float>(v[1]);
    }
};
struct ElemBF16 {   // the upper half of an fp32: shift and mask
    typedef uint16_t raw;
    static __device__ __forceinline__ float one(uint16_t b) { return __uint_as_float(static_cast<uint32_t>(b) << 16); }
    static __device__ __forceinline__ void two(uint32_t w, float& lo, float& hi) {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xffff0000u);
    }
};

template <typename E> constexpr bool kTwoByteElem = sizeof(typename E::raw) == 2;                          // fp16 / bf16, of W or of X
template <typename E> constexpr int32_t kWtype = std::is_same_v<E, ElemBF16> ? OQ_W_BF16 : OQ_W_F16;      // wtype / xtype of a 2-byte E

// f(ElemF16{}) or f(ElemBF16{}) for a type code that half_operand_ok has let through: `f` is a generic lambda, decltype of its
// argument the element type.  The only place where a type code selects an instantiation.
template <typename F>
auto with_half_elem(int32_t type, F&& f) { return type == OQ_W_BF16 ? f(ElemBF16{}) : f(ElemF16{}); }

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// What entry point `fn` checks of its 2-byte operand `name` ("W", "X" or "x"; the type argument is called after it, wtype / xtype):
// a known type code and a pointer aligned to the element.  Null is aligned: whether it is allowed stays with the entry point, and
// an entry point whose operands come in a table passes null here and checks the pointers entry by entry.
inline int32_t half_operand_ok(const char* fn, const char* name, int32_t type, const void* p) {
    OQ_REQUIRE(type == OQ_W_F16 || type == OQ_W_BF16, OQ_ERR_INVALID_ARGUMENT, "%s: unknown %ctype %d", fn, name[0] | 0x20, type);
    OQ_REQUIRE(aligned_to(p, 2), OQ_ERR_INVALID_ARGUMENT, "%s: %s must be 2-byte aligned", fn, name);
    return OQ_OK;
}

}  // namespace oq
