// What the two routes of include/oq_hip_nbits.h and include/oq_hip_nbits_decode.h share (matmul_nbits.hip, matmul_nbits_decode.hip;
// DESIGN.md 4.23, 4.26): the 2-byte matrix-core operand of an element type, the decoders of a loaded word of the blob and of a packed
// zero point, and the checks both entry points make of a call.  One text, so the two routes refuse the same calls with the same
// words and read the same blob.
#pragma once

#include "half_elem.hpp"

#include "../../include/oq_hip_nbits.h"

namespace oq {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- device: the operand of v_mfma_f32_16x16x32_f16 / _bf16.  pack: two exact integers of at most 8 bits (and a sign) as one dword of
// operands, the first in the low half; round: the one rounding of an fp32 to 2 bytes; kOnes: a dword of two ones.
struct OpF16 : ElemF16 {
    typedef f16x8 frag;
    static constexpr uint32_t kOnes = 0x3C003C00u;
    static __device__ __forceinline__ uint32_t pack(float a, float b) {      // exact integers: the rounding mode is irrelevant
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
    }
    static __device__ __forceinline__ uint16_t round(float v) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v)); }
    static __device__ __forceinline__ f32x4 mma(const frag& a, const frag& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
struct OpBF16 : ElemBF16 {
    typedef bf16x8 frag;
    static constexpr uint32_t kOnes = 0x3F803F80u;
    static __device__ __forceinline__ uint32_t pack(float a, float b) {      // |a|, |b| <= 255: eight significand bits, the upper halves
        return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
    }
    static __device__ __forceinline__ uint16_t round(float v) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v)); }
    static __device__ __forceinline__ f32x4 mma(const frag& a, const frag& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// Value i (k ascending) of a loaded word of the blob, as fp32.  A 4-bit word holds 8: byte b holds values 2 b (low nibble) and
// 2 b + 1, so the even and the odd values are each four whole bytes of a masked word.  An 8-bit word holds 4.
template <int BITS>
__device__ __forceinline__ float stored(uint32_t w, int i) {
    if constexpr (BITS == 4) return static_cast<float>((((i & 1 ? w >> 4 : w) & 0x0F0F0F0Fu) >> (8 * (i >> 1))) & 0xFFu);
    else return static_cast<float>((w >> (8 * i)) & 0xFFu);
}

// a loaded word minus the zero point -> its 32 / BITS values as 16 / BITS dwords of exact 2-byte operands
template <typename OP, int BITS>
__device__ __forceinline__ void dequant_word(uint32_t w, float zp, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < 16 / BITS; ++i) out[i] = OP::pack(stored<BITS>(w, 2 * i) - zp, stored<BITS>(w, 2 * i + 1) - zp);
}

// The packed zero point of row n, group kb: the byte that holds it (4 bits: two groups a byte, rows padded to whole bytes), and the
// zero point in that byte.
template <int BITS, typename I>      // I: the kernel's type of a group index
__device__ __forceinline__ uint32_t zp_byte(const uint8_t* zp, int64_t n, int64_t blocks, I kb) {
    return BITS == 4 ? zp[n * ((blocks + 1) >> 1) + (kb >> 1)] : zp[n * blocks + kb];
}
template <int BITS, typename I>
__device__ __forceinline__ uint32_t zp_of_byte(uint32_t byte, I kb) {
    return BITS == 4 ? (byte >> (4 * (kb & 1))) & 0xFu : byte;
}

// ---- host: the checks of a call.  What differs between the routes is named by an NbitsRoute; a check that only one route makes, in
// words of its own, stays in its file between these functions, so that a call with several faults is refused for the same one.
struct NbitsRoute {
    const char* fn;
    int64_t max_rows;              // of A
    int64_t group_unit;            // group_size is a multiple of it ...
    const char* group_why;         // ... because
    bool float_zero_points;        // have a kernel
};

inline bool type_ok(int32_t t) { return t == OQ_NBITS_F32 || t == OQ_NBITS_F16 || t == OQ_NBITS_BF16; }

// the operands both routes read and write: A [M, K] is bounded by its extents, or by what the tile route makes of it
inline bool shape_ok(int64_t M, int64_t K, int64_t N, int64_t g) {
    return extent_ok(M) && extent_ok(K) && extent_ok(N) && extent_ok(g) && count_ok(M * N) && count_ok(N * (ceil_div(K, g) * g));
}

inline int32_t operands_ok(const char* fn, const void* A, const void* B, const void* scales, const void* Y, int32_t atype, int32_t scales_type) {
    OQ_REQUIRE(A && B && scales && Y, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (A, B, scales and Y are required)", fn);
    OQ_REQUIRE(type_ok(atype), OQ_ERR_INVALID_ARGUMENT, "%s: unknown atype %d", fn, atype);
    OQ_REQUIRE(scales_type == OQ_NBITS_F32 || scales_type == atype, OQ_ERR_INVALID_ARGUMENT, "%s: scales_type %d is neither fp32 nor atype %d", fn,
               scales_type, atype);
    return OQ_OK;
}

inline int32_t extents_and_flags_ok(const NbitsRoute& r, int64_t M, int64_t K, int64_t N, int64_t lda, int64_t ldy, int32_t bits, int64_t group_size,
                                    int32_t flags) {
    const char* fn = r.fn;
    OQ_REQUIRE(extent_ok(M) && extent_ok(K) && extent_ok(N) && matrix_ok(M, K, lda) && matrix_ok(M, N, ldy), OQ_ERR_INVALID_ARGUMENT,
               "%s: M=%lld K=%lld N=%lld lda=%lld ldy=%lld outside the bounds", fn, (long long)M, (long long)K, (long long)N, (long long)lda,
               (long long)ldy);
    OQ_REQUIRE(M <= r.max_rows, OQ_ERR_UNSUPPORTED, "%s: M = %lld rows (the decode route takes 1 ... %lld; oq_matmul_nbits takes the rest)", fn,
               (long long)M, (long long)r.max_rows);
    OQ_REQUIRE(bits == 4 || bits == 8, OQ_ERR_UNSUPPORTED, "%s: bits = %d (4 and 8 have a kernel)", fn, bits);
    OQ_REQUIRE(extent_ok(group_size) && group_size % r.group_unit == 0, OQ_ERR_UNSUPPORTED, "%s: group_size = %lld is no multiple of %lld (%s)", fn,
               (long long)group_size, (long long)r.group_unit, r.group_why);
    OQ_REQUIRE(r.float_zero_points || !(flags & OQ_NBITS_FLOAT_ZERO_POINTS), OQ_ERR_UNSUPPORTED,
               "%s: float zero points (q - zp is no integer: no exact matrix-core operand)", fn);
    OQ_REQUIRE(!(flags & OQ_NBITS_G_IDX), OQ_ERR_UNSUPPORTED, "%s: g_idx has no kernel", fn);
    OQ_REQUIRE((flags & ~(OQ_NBITS_FLOAT_ZERO_POINTS | OQ_NBITS_G_IDX)) == 0, OQ_ERR_INVALID_ARGUMENT, "%s: unknown flags %d", fn, flags);
    return OQ_OK;
}

// A, Y, bias and scales are aligned to their elements
inline int32_t element_alignment_ok(const char* fn, const void* A, const void* Y, const void* bias, const void* scales, int32_t atype, int32_t scales_type) {
    const uintptr_t elem = atype == OQ_NBITS_F32 ? 4 : 2;
    OQ_REQUIRE(aligned_to(A, elem) && aligned_to(Y, elem) && aligned_to(bias, elem) && aligned_to(scales, scales_type == OQ_NBITS_F32 ? 4 : 2),
               OQ_ERR_INVALID_ARGUMENT, "%s: A, Y, bias and scales must be aligned to their element", fn);
    return OQ_OK;
}

// `ws` has carved the route's plan from (workspace, workspace_bytes)
inline int32_t workspace_ok(const char* fn, const Workspace& ws, const void* workspace, size_t workspace_bytes) {
    OQ_REQUIRE(ws.total() == 0 || ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);
    return OQ_OK;
}
inline int32_t blob_and_workspace_ok(const char* fn, const void* B, const Workspace& ws, const void* workspace, size_t workspace_bytes) {
    OQ_REQUIRE(aligned_to(B, 16), OQ_ERR_INVALID_ARGUMENT, "%s: B must be 16-byte aligned", fn);
    return workspace_ok(fn, ws, workspace, workspace_bytes);
}

}  // namespace
}  // namespace oq
