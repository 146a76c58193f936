// What the two routes of include/oq_hip_qlinear.h and include/oq_hip_qlinear_decode.h share (qlinear_gemm.hip, qlinear_decode.hip;
// DESIGN.md 4.24, 4.27).  Device: the guarded loads of an 8-bit operand, the terms of the zero-point correction that belong to an
// output column, and the epilogue -- acc -> Y in the order the headers state, every fp32 step one rounding.  Host (at the end): the
// checks of a call and the operand block of the argument structs.  One text, so the two routes give the same bytes and refuse the
// same calls with the same words.  qlinear_function.hip (include/oq_hip_qlinear_function.h) runs the same routes on
// an fp32 A and to an fp32 Y: its quantizer (quant_k16, a drop-in for load_k16) and the dequantizing step of finish_acc are here too.
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

// acc -> Y.  Every fp32 step is one rounding, in the order the header states.  DQ (include/oq_hip_qlinear_function.h; the 8-bit
// output codes only): Y is fp32 and takes the dequantized value (fp32(q) - fp32(y_zp)) * y_scale in the place of q -- q is an
// integer of the type's range held in fp32, so no conversion lies between.
template <bool DQ = false, class P>
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
    if constexpr (DQ) {
        static_cast<float*>(p.Y)[at] = (q - static_cast<float>(read_zp(p.y_zp, i8, 0))) * p.y_scale[0];
        return;
    }
    static_cast<uint8_t*>(p.Y)[at] = static_cast<uint8_t>(static_cast<int32_t>(q));
}

// S -> acc -> Y, for a kernel whose row sums lie in memory
template <bool DQ = false, class P>
__device__ __forceinline__ void finish(const P& p, uint32_t m, uint32_t n, uint32_t S, const ColTerms& c) {
    const uint32_t rs = p.rowsum ? static_cast<uint32_t>(p.rowsum[m]) : 0u;
    finish_acc<DQ>(p, m, n, static_cast<int32_t>(S - c.zb * rs + c.add), c.scale);
}

// What the tile bodies (qlinear_tile.hpp) end in: the 8-bit q, its dequantized value (the DQ of finish_acc), or the epilogue of a QDQ
// function with quantized activations (include/oq_hip_qdq_function.h).
enum : int { kEpQuantized = 0, kEpDequantized = 1, kEpQdqFunction = 2 };
// the modes of an activation, as oq_qdq_mode numbers them (the header is not included here: it would pull the whole QDQ vocabulary in)
enum : int { kQdqNone = 0, kQdqStatic = 1, kQdqDynamic = 2 };

// a running (min, max) that propagates NaN; the identity of both folds
struct MinMax {
    float lo = __builtin_inff(), hi = -__builtin_inff();
};

// DynamicQuantizeLinear's parameters from the (min, max) of a tensor, and its element function (include/oq_hip_qdq_function.h)
struct DynParams {
    float safe, scale, zp;
};
__device__ __forceinline__ DynParams dyn_params(const MinMax& t) {
    const float lo = nmin(t.lo, 0.0f), hi = nmax(t.hi, 0.0f);
    DynParams d;
    d.scale = (hi - lo) / 255.0f;
    d.safe = d.scale == 0.0f ? 1.0f : d.scale;
    d.zp = rintf(fminf(fmaxf(-lo / d.safe, 0.0f), 255.0f));
    return d;
}
__device__ __forceinline__ float dyn_qdq(float t, const DynParams& d) {
    const float q = fminf(fmaxf(rintf(t / d.safe) + d.zp, 0.0f), 255.0f);
    return (q - d.zp) * d.scale;
}

// the dequantized bias of a Gemm for column n (0 for a MatMul).  `P` also names bias, bias_scale, bias_zp.
template <class P>
__device__ __forceinline__ float qdq_bias(const P& p, uint32_t n) {
    if (!p.bias) return 0.0f;
    return (static_cast<float>(p.bias[n]) - static_cast<float>(p.bias_zp ? p.bias_zp[0] : 0)) * p.bias_scale[0];
}

// S -> v -> Y for kEpQdqFunction.  `P` also names out_mode and out_signed; y_scale / y_zp are the static output parameters.  A
// dynamic output takes v as it is and folds it into `mm`: the finishing launch rewrites Y.
template <class P>
__device__ __forceinline__ void finish_qdq(const P& p, uint32_t m, uint32_t n, uint32_t S, const ColTerms& c, float bias, MinMax& mm) {
    const uint32_t rs = p.rowsum ? static_cast<uint32_t>(p.rowsum[m]) : 0u;
    float v = static_cast<float>(static_cast<int32_t>(S - c.zb * rs + c.add)) * c.scale;
    if (p.bias) v = v + bias;
    float* const y = static_cast<float*>(p.Y) + static_cast<int64_t>(m) * p.ldy + n;
    if (p.out_mode == kQdqStatic && v == v) {      // a NaN (a dynamic input that holds one) passes
        const float zp = static_cast<float>(read_zp(p.y_zp, p.out_signed, 0));
        const float q = fminf(fmaxf(rintf(v / p.y_scale[0]) + zp, p.out_signed ? -128.0f : 0.0f), p.out_signed ? 127.0f : 255.0f);
        v = (q - zp) * p.y_scale[0];
    }
    if (p.out_mode == kQdqDynamic) mm.lo = nmin(mm.lo, v), mm.hi = nmax(mm.hi, v);
    *y = v;
}

// the fold of a wave's MinMax: every lane gets the result (min and max are exact in any order)
__device__ __forceinline__ MinMax wave_minmax(MinMax mm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mm.lo = nmin(mm.lo, __shfl_xor(mm.lo, off, kWave));
        mm.hi = nmax(mm.hi, __shfl_xor(mm.hi, off, kWave));
    }
    return mm;
}

// the fold of a workgroup's MinMax, which every thread of it calls: every thread gets the result.  `red`: 2 floats per wave of LDS
// that nobody reads any more.
__device__ __forceinline__ MinMax block_minmax(MinMax mm, float* red) {
    mm = wave_minmax(mm);
    if ((threadIdx.x & 63) == 0) red[2 * (threadIdx.x >> 6)] = mm.lo, red[2 * (threadIdx.x >> 6) + 1] = mm.hi;
    __syncthreads();
    MinMax all;
    for (unsigned w = 0; w < blockDim.x / kWave; ++w) all.lo = nmin(all.lo, red[2 * w]), all.hi = nmax(all.hi, red[2 * w + 1]);
    return all;
}

// ... and into pairs[2 * block], pairs[2 * block + 1], as one 8-byte store
__device__ __forceinline__ void block_minmax_store(const MinMax& mm, float* red, float* pairs, uint32_t block) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const MinMax all = block_minmax(mm, red);
    if (threadIdx.x == 0) *reinterpret_cast<f32x2*>(pairs + 2 * static_cast<int64_t>(block)) = f32x2{all.lo, all.hi};
}

// QuantizeLinear of an fp32 operand to an 8-bit type, per tensor (include/oq_hip_qlinear_function.h): what one element needs.
struct QuantParams {
    float scale, zp, lo, hi;
};

// of operand A of an argument block: a_scale, a_zp (NULL: 0) and the range of A's type
template <class P>
__device__ __forceinline__ QuantParams quant_of(const P& p) {
    return QuantParams{p.a_scale[0], static_cast<float>(read_zp(p.a_zp, p.a_signed, 0)), p.a_signed ? -128.0f : 0.0f, p.a_signed ? 127.0f : 255.0f};
}

// q = sat(rint(x / scale) + zp) as the low byte of a dword: one IEEE division, rint to even, one addition, the clamp in fp32, then
// the conversion.  +-inf and quotients beyond the range saturate; a NaN gives the bottom of the type (fmaxf returns its other operand),
// as finish_acc does.  Not oq_common.hpp's quantize_one, which converts to int32 ahead of the zero point.
__device__ __forceinline__ uint32_t quant_byte(float x, const QuantParams& q) {
    const float v = fminf(fmaxf(rintf(x / q.scale) + q.zp, q.lo), q.hi);
    return static_cast<uint32_t>(static_cast<int32_t>(v)) & 0xFFu;
}

// load_k16 for an fp32 row that is quantized on the way: 16 raw bytes of the 8-bit operand for k ... k + 15, past K the flip's byte.
// No float at or beyond k = K is read.  `vec`: the row is 16-byte aligned (four 16-byte loads where the chunk lies inside K).
__device__ __forceinline__ u32x4 quant_k16(const float* row, uint32_t k, uint32_t K, bool vec, const QuantParams& q, uint32_t flip) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    uint32_t w[4];
    if (vec && k + 16u <= K) {
        f32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(row + k + 4 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) w[j] |= quant_byte(x[j][b], q) << (8 * b);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t kk = k + 4 * j + b;
                w[j] |= (kk < K ? quant_byte(row[kk], q) : flip & 0xFFu) << (8 * b);
            }
        }
    }
    return u32x4{w[0], w[1], w[2], w[3]};
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

// ---- host: the front of both entry points -- what they require of a call, and the operand block of their argument structs
inline bool type_ok(int32_t t) { return t == OQ_QL_U8 || t == OQ_QL_I8; }
inline bool layout_ok(int32_t l) { return l == OQ_QL_KN || l == OQ_QL_NK; }

inline bool shape_ok(int64_t M, int64_t K, int64_t N) {
    return extent_ok(M) && extent_ok(K) && extent_ok(N) && count_ok(M * K) && count_ok(M * N) && count_ok(N * K);
}

// `max_rows`: of the route `fn` (the tile route: any number an extent can be)
inline int32_t call_ok(const char* fn, int64_t max_rows, const void* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                       const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale, const int32_t* C,
                       const float* y_scale, int32_t flags, int32_t out, const void* Y, int64_t ldy) {
    OQ_REQUIRE(A && B && Y, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (A, B and Y are required)", fn);
    OQ_REQUIRE(type_ok(a_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown a_type %d", fn, a_type);
    OQ_REQUIRE(type_ok(b_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown b_type %d", fn, b_type);
    OQ_REQUIRE(layout_ok(b_layout), OQ_ERR_INVALID_ARGUMENT, "%s: unknown b_layout %d", fn, b_layout);
    OQ_REQUIRE(out == OQ_QL_OUT_I32 || out == OQ_QL_OUT_F32 || out == OQ_QL_OUT_U8 || out == OQ_QL_OUT_I8, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown out %d", fn, out);
    OQ_REQUIRE((flags & ~(OQ_QL_PER_ROW_A | OQ_QL_TRANS_A | OQ_QL_ALPHA)) == 0, OQ_ERR_INVALID_ARGUMENT, "%s: unknown flags %d", fn, flags);
    OQ_REQUIRE(out == OQ_QL_OUT_I32 || (a_scale && b_scale), OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (a_scale and b_scale are required for out %d)",
               fn, out);
    OQ_REQUIRE((out != OQ_QL_OUT_U8 && out != OQ_QL_OUT_I8) || y_scale, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (y_scale is required for out %d)",
               fn, out);
    const bool kn = b_layout == OQ_QL_KN;
    OQ_REQUIRE(extent_ok(M) && extent_ok(K) && extent_ok(N) && matrix_ok(M, K, lda) && matrix_ok(kn ? K : N, kn ? N : K, ldb) && matrix_ok(M, N, ldy),
               OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld lda=%lld ldb=%lld ldy=%lld outside the bounds", fn, (long long)M, (long long)K,
               (long long)N, (long long)lda, (long long)ldb, (long long)ldy);
    OQ_REQUIRE(shape_ok(M, K, N), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld: an operand beyond 2^40 elements", fn, (long long)M,
               (long long)K, (long long)N);
    OQ_REQUIRE(M <= max_rows, OQ_ERR_UNSUPPORTED, "%s: M = %lld rows (the decode route takes 1 ... %lld; oq_qlinear_matmul is the route)", fn,
               (long long)M, (long long)max_rows);
    OQ_REQUIRE(!(flags & OQ_QL_PER_ROW_A), OQ_ERR_UNSUPPORTED, "%s: per-row a_scale / a_zero_point have no kernel", fn);
    OQ_REQUIRE(!(flags & OQ_QL_TRANS_A), OQ_ERR_UNSUPPORTED, "%s: transA has no kernel", fn);
    OQ_REQUIRE(!(flags & OQ_QL_ALPHA), OQ_ERR_UNSUPPORTED, "%s: alpha != 1 has no kernel", fn);
    OQ_REQUIRE(aligned_to(a_scale, 4) && aligned_to(b_scale, 4) && aligned_to(y_scale, 4) && aligned_to(C, 4) &&
                   aligned_to(Y, out == OQ_QL_OUT_I32 || out == OQ_QL_OUT_F32 ? 4 : 1),
               OQ_ERR_INVALID_ARGUMENT, "%s: the scales, C and Y must be aligned to their element", fn);
    return OQ_OK;
}

// a sum is needed unless its multiplier -- the OTHER operand's shifted zero point -- is zero whatever the device holds
inline bool sum_needed(int32_t other_signed, const void* other_zero_point) { return !(other_signed && !other_zero_point); }

// the fields A ... ldy, M, N, K of an argument block, from a call that call_ok has let through
template <class P>
void fill_operands(P& p, const void* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale, const void* a_zero_point,
                   const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point,
                   int32_t b_per_column, const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t out, void* Y, int64_t ldy) {
    p.A = static_cast<const uint8_t*>(A), p.B = static_cast<const uint8_t*>(B);
    p.lda = lda, p.ldb = ldb;
    p.a_signed = a_type == OQ_QL_I8, p.b_signed = b_type == OQ_QL_I8;
    p.a_flip = p.a_signed ? 0u : 0x80808080u, p.b_flip = p.b_signed ? 0u : 0x80808080u;
    p.a_vec = aligned_to(A, 16) && lda % 16 == 0;
    p.b_vec = b_layout == OQ_QL_KN ? (aligned_to(B, 4) && ldb % 4 == 0) : (aligned_to(B, 16) && ldb % 16 == 0);
    p.a_scale = a_scale, p.a_zp = a_zero_point, p.b_scale = b_scale, p.b_zp = b_zero_point, p.b_per_column = b_per_column != 0;
    p.C = C, p.y_scale = y_scale, p.y_zp = y_zero_point, p.out = out, p.Y = Y, p.ldy = ldy;
    p.M = static_cast<uint32_t>(M), p.N = static_cast<uint32_t>(N), p.K = static_cast<uint32_t>(K);
}

}  // namespace
}  // namespace oq
