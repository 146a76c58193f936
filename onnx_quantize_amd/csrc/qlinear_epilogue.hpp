// What the kernels of include/oq_hip_qlinear.h and include/oq_hip_qlinear_decode.h share (qlinear_gemm.hip, qlinear_decode.hip;
// DESIGN.md 4.24, 4.27): the guarded loads of an 8-bit operand, the terms of the zero-point correction that belong to an output
// column, and the epilogue -- acc -> Y in the order the headers state, every fp32 step one rounding.  One text, so the two routes
// give the same bytes.
//
// `P` is a kernel's argument block.  It names a_zp, a_signed, b_zp, b_signed, b_per_column, a_scale, b_scale, C, K (col_terms: also
// colsum, colsum_slices, colsum_stride), and y_scale, y_zp, out, Y, ldy (finish: also rowsum).
#pragma once

#include "half_elem.hpp"

#include "../../include/oq_hip_qlinear.h"

namespace oq {
namespace {

__device__ __forceinline__ int32_t read_zp(const void* zp, int32_t is_signed, int64_t i) {
    if (zp == nullptr) return 0;
    return is_signed ? static_cast<int32_t>(static_cast<const int8_t*>(zp)[i]) : static_cast<int32_t>(static_cast<const uint8_t*>(zp)[i]);
}

// the shifted zero points of the flipped operands: za' = a_zp - 128 [A unsigned], zb'[n] likewise
template <class P>
__device__ __forceinline__ uint32_t shifted_a_zp(const P& p) {
    return static_cast<uint32_t>(read_zp(p.a_zp, p.a_signed, 0) - (p.a_signed ? 0 : 128));
}
template <class P>
__device__ __forceinline__ uint32_t shifted_b_zp(const P& p, uint32_t n) {
    return static_cast<uint32_t>(read_zp(p.b_zp, p.b_signed, p.b_per_column ? n : 0) - (p.b_signed ? 0 : 128));
}
// fl(a_scale * b_scale[n]); not read for OQ_QL_OUT_I32, whose scales may be NULL
template <class P>
__device__ __forceinline__ float out_scale(const P& p, uint32_t n) {
    return p.out == OQ_QL_OUT_I32 ? 0.0f : p.a_scale[0] * p.b_scale[p.b_per_column ? n : 0];
}

// what an output column needs: zb'[n], the terms of the correction that do not depend on the row, and the fp32 scale
struct ColTerms {
    uint32_t zb, add;
    float scale;
};

// (the zero points and the scale are spelled out, not taken from the helpers above: with them the compiler orders the loads of the
// tile kernels differently, and scripts/compare_kernel_asm.py holds those kernels to their text)
template <class P>
__device__ __forceinline__ ColTerms col_terms(const P& p, uint32_t n) {
    ColTerms c;
    const uint32_t za = static_cast<uint32_t>(read_zp(p.a_zp, p.a_signed, 0) - (p.a_signed ? 0 : 128));
    c.zb = static_cast<uint32_t>(read_zp(p.b_zp, p.b_signed, p.b_per_column ? n : 0) - (p.b_signed ? 0 : 128));
    c.add = p.K * za * c.zb;
    if (p.colsum) {
        uint32_t cs = 0u;
        for (uint32_t s = 0; s < p.colsum_slices; ++s) cs += static_cast<uint32_t>(p.colsum[static_cast<int64_t>(s) * p.colsum_stride + n]);
        c.add -= za * cs;
    }
    if (p.C) c.add += static_cast<uint32_t>(p.C[n]);
    c.scale = p.out == OQ_QL_OUT_I32 ? 0.0f : p.a_scale[0] * p.b_scale[p.b_per_column ? n : 0];
    return c;
}

// acc -> Y.  Every fp32 step is one rounding, in the order the header states.
template <class P>
__device__ __forceinline__ void finish_acc(const P& p, uint32_t m, uint32_t n, int32_t acc, float scale) {
    const int64_t at = static_cast<int64_t>(m) * p.ldy + n;
    if (p.out == OQ_QL_OUT_I32) {
        static_cast<int32_t*>(p.Y)[at] = acc;
        return;
    }
    const float t = static_cast<float>(acc) * scale;
    if (p.out == OQ_QL_OUT_F32) {
        static_cast<float*>(p.Y)[at] = t;
        return;
    }
    const bool i8 = p.out == OQ_QL_OUT_I8;
    float q = rintf(t / p.y_scale[0]) + static_cast<float>(read_zp(p.y_zp, i8, 0));
    q = fminf(fmaxf(q, i8 ? -128.0f : 0.0f), i8 ? 127.0f : 255.0f);
    static_cast<uint8_t*>(p.Y)[at] = static_cast<uint8_t>(static_cast<int32_t>(q));
}

// S -> acc -> Y, for a kernel whose row sums lie in memory
template <class P>
__device__ __forceinline__ void finish(const P& p, uint32_t m, uint32_t n, uint32_t S, const ColTerms& c) {
    const uint32_t rs = p.rowsum ? static_cast<uint32_t>(p.rowsum[m]) : 0u;
    finish_acc(p, m, n, static_cast<int32_t>(S - c.zb * rs + c.add), c.scale);
}

// 16 bytes of `row` from k on, as they are: the flip is applied by whoever consumes them, so that no load is followed by an
// instruction that waits for it.  Past K: the flip's byte, which the flip turns into the pad, a zero of the flipped operand.
__device__ __forceinline__ u32x4 load_k16(const uint8_t* row, uint32_t k, uint32_t K, bool vec, uint32_t flip) {
    if (vec && k + 16u <= K) return *reinterpret_cast<const u32x4*>(row + k);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w[j] = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t kk = k + 4 * j + b;
            w[j] |= (kk < K ? static_cast<uint32_t>(row[kk]) : flip & 0xFFu) << (8 * b);
        }
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// 4 bytes of one row of a KN matrix from column n on, `at` pointing at column n (raw; zeros past N)
__device__ __forceinline__ uint32_t load_n4(const uint8_t* at, uint32_t n, uint32_t N, bool vec) {
    if (vec && n + 4u <= N) return *reinterpret_cast<const uint32_t*>(at);
    uint32_t w = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (n + b < N) w |= static_cast<uint32_t>(at[b]) << (8 * b);
    return w;
}

}  // namespace
}  // namespace oq
