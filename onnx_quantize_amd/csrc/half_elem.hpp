// The fp16 / bf16 element of the half-precision sources (rtn_half.hip, hqq.hip, reduce_half.hip, abs_stats_half.hip): the exact
// conversion to fp32 at the load, the words a lane loads them in, and the two host tests every half entry point makes.
#pragma once

#include <cstdint>
#include <type_traits>

#include "oq_common.hpp"

#include "../../include/oq_hip_half.h"

namespace oq {

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
// for the kernels that are templates on `bool BF16`
template <bool BF16> using HalfElem = std::conditional_t<BF16, ElemBF16, ElemF16>;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

inline bool half_type_ok(int32_t type) { return type == OQ_W_F16 || type == OQ_W_BF16; }                                // wtype / xtype
inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }   // n: a power of two

}  // namespace oq
