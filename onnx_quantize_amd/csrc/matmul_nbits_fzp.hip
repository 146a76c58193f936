// com.microsoft::MatMulNBits with FLOATING-POINT zero points (HQQ files), any M, run from the packed blob
// (include/oq_hip_nbits_fzp.h):
//
//       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
//
// q - zp is no integer here, so it is no exact matrix-core operand.  Every zero point is split once, where it is staged:
//       zi = clamp(rint(zp), 0, 2^bits - 1)          f = zp - zi          (fp32; |f| <= 0.5 while zp lies inside the type's range)
// q - zi is the integer in [-255, 255] that matmul_nbits.hip stages, through the same decoders, and per group
//       sum_k a (q - zp) = sum_k a (q - zi) - f sum_k a:      t = fma(-f, rs, acc),  sum = fma(t, scale, sum)
// with acc the group's MFMA accumulator and rs the sums of A's rows over the same k.  rs comes from the matrix cores: one more MFMA
// per fragment of A against a fragment of ones (tile_gemm, kFloatZp), which leaves the sums of exactly the rows a lane's accumulators
// hold in all 16 columns, reset where acc is reset and cut by the same split of K: no workspace, no launch and no pass over A of its
// own.  Splitting at rint(zp) and not at 0 keeps the cancellation between sum a (q - zi) and f sum a, where |f| <= 0.5, and not
// between sum a q and zp sum a, where zp sits mid-range.
//
// The tile, the plan, the workspace, the fp32-A pieces, the split of K, the guards and the GEMM body are matmul_nbits.hip's: tile_gemm,
// make_plan and run_for_a of nbits_tile.hpp, the checks of nbits_common.hpp.  This file's own are the staging policy (FzpStage: the
// blob as BlobStage reads it, the zero point as a float, its fraction and the scale through 2 KiB of LDS to the lanes that fold) and the entry
// point.  A zero point outside [0, 2^bits - 1] is legal: zi is clamped and f takes the rest.  A NaN zero point gives zi = 0 and f = NaN:
// exactly its column of Y is NaN.
// Built with -fno-slp-vectorize (_build.py), like its three siblings and for their reason: no v_pk_fma_f32 folds (docs/LAB_NOTES_r22.md).
#include "nbits_tile.hpp"
#include "tile_plan.hpp"

#include "../../include/oq_hip_nbits_fzp.h"

namespace oq {
namespace {

struct FzpArgs : NbitsArgs {      // zp: [N, blocks] floats
    int32_t zp_f32;               // fp32, or 2 bytes of A's type
};

// tile_gemm's staging policy: BlobStage of matmul_nbits.hip with a floating-point zero point.  Thread t stages 32 values of row
// t >> 1 of the step (half t & 1 of its 64 k) and that half's zero point; a 32-deep half lies in one group (g % 32 == 0).
template <int BITS>
struct FzpStage {
    typedef FzpArgs args;
    static constexpr int kRows = kBN, kFragStride = 16;
    static constexpr bool kFloatZp = true;
    static __device__ __forceinline__ int frag_row(int wn, int lane) { return wn * 64 + (lane & 15); }
    static __device__ __forceinline__ int64_t group(const FzpArgs& p, int64_t k) { return k / p.g; }
    static __device__ __forceinline__ int64_t within(const FzpArgs& p, int64_t k) { return k % p.g; }

    // (f, scale) of [half of the step][column of the tile], written with the operands of a step and read between the step's two
    // barriers by the lanes that fold that column
    static __device__ __forceinline__ u32x2* terms() {
        __shared__ u32x2 t[2 * kBN];
        return t;
    }
    static __device__ __forceinline__ void group_terms(int s, int wn, int lane, float (&fz)[4], float (&sc)[4]) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const u32x2 t = terms()[s * kBN + wn * 64 + (lane & 15) + 16 * nt];
            fz[nt] = __uint_as_float(t[0]), sc[nt] = __uint_as_float(t[1]);
        }
    }

    u32x4 b_regs[BITS / 4];
    uint32_t zp_raw = 0, sc_raw = 0;      // the staged group's zero point and scale as loaded (0: a column past N, a half past the block's k)
    const int b_row, b_half;
    const int64_t b_n;

    __device__ __forceinline__ FzpStage(const FzpArgs&, int tid, int64_t n0) : b_row(tid >> 1), b_half(tid & 1), b_n(n0 + b_row) {}

    __device__ __forceinline__ void load(const FzpArgs& p, int64_t k, int64_t, int64_t k_end) {
        const int64_t kb_k = k + 32 * b_half;
#pragma unroll
        for (int i = 0; i < BITS / 4; ++i) b_regs[i] = u32x4{0u, 0u, 0u, 0u};
        zp_raw = sc_raw = 0u;
        if (b_n < p.N && kb_k < k_end) {      // B and the zero points past N or K are never read
            const int64_t kb = kb_k / p.g, in_kb = kb_k - kb * p.g;
            const uint8_t* src = p.B + ((b_n * p.blocks + kb) * p.g + in_kb) * BITS / 8;
#pragma unroll
            for (int i = 0; i < BITS / 4; ++i) b_regs[i] = reinterpret_cast<const u32x4*>(src)[i];
            const int64_t at = b_n * p.blocks + kb;
            zp_raw = p.zp_f32 ? reinterpret_cast<const uint32_t*>(p.zp)[at] : reinterpret_cast<const uint16_t*>(p.zp)[at];
            sc_raw = p.scales_f32 ? static_cast<const uint32_t*>(p.scales)[at] : static_cast<const uint16_t*>(p.scales)[at];
        }
    }
    template <typename OP>
    __device__ __forceinline__ void store(const FzpArgs& p, unsigned char* lds_b) const {
        const float zp = p.zp_f32 ? __uint_as_float(zp_raw) : OP::one(static_cast<uint16_t>(zp_raw));
        const float top = static_cast<float>((1 << BITS) - 1), r = rintf(zp);
        const float zi = r > 0.0f ? (r < top ? r : top) : 0.0f;      // a NaN: 0, and f = NaN
        const float sc = p.scales_f32 ? __uint_as_float(sc_raw) : OP::one(static_cast<uint16_t>(sc_raw));
        terms()[b_half * kBN + b_row] = u32x2{__float_as_uint(zp - zi), __float_as_uint(sc)};
        u32x4 d[4];
        dequant32<OP, BITS>(b_regs, zi, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(lds_b + b_row * kRow + b_half * 64 + i * 16) = d[i];
    }
};

// Two waves per SIMD for a 2-byte A, one for an fp32 A, as matmul_nbits.hip's kernels and for its reasons.
template <int OUT, int BITS, int MT>
__global__ __launch_bounds__(kThreads, OUT == OQ_NBITS_F32 ? 1 : 2) void nbits_fzp_gemm_kernel(const FzpArgs p) { tile_gemm<OUT, MT, FzpStage<BITS>>(p); }

// ---- host
constexpr NbitsRoute kRoute{"oq_matmul_nbits_fzp", kMaxExtent, 32, "two groups would share one 32-deep matrix instruction", true};

template <int OUT, int BITS>
void launch_gemm(const FzpArgs& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { nbits_fzp_gemm_kernel<OUT, BITS, decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
}

template <int OUT>
int32_t run(const FzpArgs& p, const Plan& pl, int32_t bits, hipStream_t s) {
    if (bits == 4) launch_gemm<OUT, 4>(p, pl, s);
    else launch_gemm<OUT, 8>(p, pl, s);
    const int32_t st = check_launch("nbits_fzp_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    return reduce_slabs<OUT>(p, pl, s);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_nbits_fzp_extension_version(void) { return OQ_NBITS_FZP_EXTENSION_VERSION; }

size_t oq_matmul_nbits_fzp_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype) {
    return plan_workspace_bytes(M, K, N, group_size, atype, [&] {
        set_error("oq_matmul_nbits_fzp_workspace_bytes: M=%lld K=%lld N=%lld group_size=%lld atype=%d outside the bounds", (long long)M, (long long)K,
                  (long long)N, (long long)group_size, atype);
    });
}

int32_t oq_matmul_nbits_fzp(const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, const void* B, int32_t bits, int64_t N, int64_t group_size,
                            const void* scales, int32_t scales_type, const void* zero_points, int32_t zero_points_type, const void* bias, int32_t flags,
                            void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = kRoute.fn;
    int32_t st = operands_ok(fn, A, B, scales, Y, atype, scales_type);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(zero_points_type == OQ_NBITS_ZP_PACKED_U8 || zero_points_type == OQ_NBITS_F32 || zero_points_type == atype, OQ_ERR_INVALID_ARGUMENT,
               "%s: zero_points_type %d is neither packed uint8 (%d), fp32 nor atype %d", fn, zero_points_type, OQ_NBITS_ZP_PACKED_U8, atype);
    st = extents_and_flags_ok(kRoute, M, K, N, lda, ldy, bits, group_size, flags);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(zero_points && zero_points_type != OQ_NBITS_ZP_PACKED_U8, OQ_ERR_UNSUPPORTED,
               "%s: integer zero points (%s): oq_matmul_nbits is their route", fn, zero_points ? "packed uint8" : "NULL");
    OQ_REQUIRE(tile_shape_ok(M, K, N, group_size), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld group_size=%lld: an operand beyond 2^40 elements", fn,
               (long long)M, (long long)K, (long long)N, (long long)group_size);
    st = element_alignment_ok(fn, A, Y, bias, scales, atype, scales_type);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(aligned_to(zero_points, zero_points_type == OQ_NBITS_F32 ? 4 : 2), OQ_ERR_INVALID_ARGUMENT, "%s: zero_points must be aligned to their element", fn);
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, atype, ws);
    st = blob_and_workspace_ok(fn, B, ws, workspace, workspace_bytes);
    if (st != OQ_OK) return st;

    hipStream_t s = as_stream(stream);
    FzpArgs p{};
    fill_args(p, scales, scales_type, zero_points, bias, Y, ldy, M, N, K, pl);
    p.zp_f32 = zero_points_type == OQ_NBITS_F32;
    p.B = static_cast<const uint8_t*>(B);
    p.g = group_size, p.blocks = ceil_div(K, group_size);
    return run_for_a(p, pl, A, atype, M, K, lda, s, [&](auto out) { return run<decltype(out)::value>(p, pl, bits, s); });
}

}  // extern "C"
