// com.microsoft::MatMulNBits run from the packed blob (include/oq_hip_nbits.h):
//
//       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
//
// q - zp is an integer in [-255, 255] and so exact in fp16 and bf16: per k-group the product A_g . (q - zp)_g runs on
// v_mfma_f32_16x16x32_f16 / _bf16 with an exact B operand into an fp32 accumulator, which is then folded into the running sum with the
// group's fp32 scale (one fma per group and output element).  The [N, K] weight never exists, in memory or in LDS: a workgroup
// dequantizes the 128 x 64 integers of its current k-step into LDS, as 2-byte operands, and nothing else.
//
// The tile, the operand layout in LDS, the register staging, the fp32-A pieces, the split of K, the guards and the GEMM body itself
// are tile_gemm in nbits_tile.hpp (the [K, N] byte-matrix GEMM, qdq_matmul.hip, keeps a copy of it).  What is this file's own is how the
// blob reaches LDS (BlobStage): a padded blob position meets a zero of A, and its bytes are finite integers whatever they hold.
// The matrix-core operand, the decoders of the blob and of a packed zero point, and the checks of a call are those of the decode
// route too: nbits_common.hpp.  The argument block, the rounding, the reduce and split-rows kernels, the plan and its workspace and
// the host tail of a call come from nbits_tile.hpp as well; its make_plan lays the workspace out around make_tile_plan(M, K, N).
#include "nbits_tile.hpp"
#include "tile_plan.hpp"

namespace oq {
namespace {

// How B reaches LDS (tile_gemm's staging policy): thread t stages 32 values of row t >> 1 of the step, as they lie in the blob, and
// writes them as row t >> 1 of a [128 columns][64 k] image.
template <int BITS>
struct BlobStage {
    typedef NbitsArgs args;
    static constexpr int kRows = kBN, kFragStride = 16;
    static constexpr bool kFloatZp = false;
    static __device__ __forceinline__ int frag_row(int wn, int lane) { return wn * 64 + (lane & 15); }
    static __device__ __forceinline__ int64_t group(const NbitsArgs& p, int64_t k) { return k / p.g; }
    static __device__ __forceinline__ int64_t within(const NbitsArgs& p, int64_t k) { return k % p.g; }

    u32x4 b_regs[BITS / 4];
    uint32_t zp_raw = 0;      // the staged group's zero point, converted where it is used: no wait for it in front of the MFMAs
    const int b_row, b_half;
    const int64_t b_n;

    __device__ __forceinline__ BlobStage(const NbitsArgs&, int tid, int64_t n0) : b_row(tid >> 1), b_half(tid & 1), b_n(n0 + b_row) {}

    __device__ __forceinline__ void load(const NbitsArgs& p, int64_t k, int64_t, int64_t k_end) {
        const int64_t kb_k = k + 32 * b_half;
#pragma unroll
        for (int i = 0; i < BITS / 4; ++i) b_regs[i] = u32x4{0u, 0u, 0u, 0u};
        zp_raw = 1u << (BITS - 1);
        if (b_n < p.N && kb_k < k_end) {      // B and the zero points past N or K are never read
            const int64_t kb = kb_k / p.g, in_kb = kb_k - kb * p.g;
            const uint8_t* src = p.B + ((b_n * p.blocks + kb) * p.g + in_kb) * BITS / 8;
#pragma unroll
            for (int i = 0; i < BITS / 4; ++i) b_regs[i] = reinterpret_cast<const u32x4*>(src)[i];
            if (p.zp != nullptr) {
                zp_raw = zp_byte<BITS>(p.zp, b_n, p.blocks, kb);      // shifted here, masked where it is used (store), not by zp_of_byte
                if constexpr (BITS == 4) zp_raw >>= 4 * (kb & 1);
            }
        }
    }
    template <typename OP>
    __device__ __forceinline__ void store(const NbitsArgs&, unsigned char* lds_b) const {
        u32x4 d[4];
        dequant32<OP, BITS>(b_regs, static_cast<float>(zp_raw & ((1u << BITS) - 1)), d);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(lds_b + b_row * kRow + b_half * 64 + i * 16) = d[i];
    }
};

// Two waves per SIMD (<= 256 registers, no scratch) for a 2-byte A: unbounded, the 128-row tile takes 230 VGPRs + 64 AGPRs, one wave
// per SIMD, and runs at less than half the speed (0.92 against 0.42 ms at 2048 x 4096 x 11008).  The fp32-A kernels stage two A pieces
// and keep one wave per SIMD (the 8-bit one needs scratch under the bound).
// This file is built with -fno-slp-vectorize (_build.py): paired, the fold of tile_gemm becomes v_pk_fma_f32 with an op_sel on the scale
// pair, which on the MI355X gave wrong low halves in lanes 48 .. 63 whenever several waves shared a SIMD (docs/LAB_NOTES_r22.md).
template <int OUT, int BITS, int MT>
__global__ __launch_bounds__(kThreads, OUT == OQ_NBITS_F32 ? 1 : 2) void nbits_gemm_kernel(const NbitsArgs p) { tile_gemm<OUT, MT, BlobStage<BITS>>(p); }

// ---- host
constexpr NbitsRoute kRoute{"oq_matmul_nbits", kMaxExtent, 32, "two groups would share one 32-deep matrix instruction", false};

template <int OUT, int BITS>
void launch_gemm(const NbitsArgs& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { nbits_gemm_kernel<OUT, BITS, decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
}

template <int OUT>
int32_t run(const NbitsArgs& p, const Plan& pl, int32_t bits, hipStream_t s) {
    if (bits == 4) launch_gemm<OUT, 4>(p, pl, s);
    else launch_gemm<OUT, 8>(p, pl, s);
    const int32_t st = check_launch("nbits_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    return reduce_slabs<OUT>(p, pl, s);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_nbits_extension_version(void) { return OQ_NBITS_EXTENSION_VERSION; }

size_t oq_matmul_nbits_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int32_t atype) {
    return plan_workspace_bytes(M, K, N, group_size, atype, [&] {
        set_error("oq_matmul_nbits_workspace_bytes: M=%lld K=%lld N=%lld group_size=%lld atype=%d outside the bounds", (long long)M, (long long)K,
                  (long long)N, (long long)group_size, atype);
    });
}

int32_t oq_matmul_nbits(const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, const void* B, int32_t bits, int64_t N, int64_t group_size,
                        const void* scales, int32_t scales_type, const uint8_t* zero_points, const void* bias, int32_t flags, void* Y, int64_t ldy,
                        void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = kRoute.fn;
    int32_t st = operands_ok(fn, A, B, scales, Y, atype, scales_type);
    if (st != OQ_OK) return st;
    st = extents_and_flags_ok(kRoute, M, K, N, lda, ldy, bits, group_size, flags);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(tile_shape_ok(M, K, N, group_size), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld group_size=%lld: an operand beyond 2^40 elements", fn,
               (long long)M, (long long)K, (long long)N, (long long)group_size);
    st = element_alignment_ok(fn, A, Y, bias, scales, atype, scales_type);
    if (st != OQ_OK) return st;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, atype, ws);
    st = blob_and_workspace_ok(fn, B, ws, workspace, workspace_bytes);
    if (st != OQ_OK) return st;

    hipStream_t s = as_stream(stream);
    NbitsArgs p{};
    fill_args(p, scales, scales_type, zero_points, bias, Y, ldy, M, N, K, pl);
    p.B = static_cast<const uint8_t*>(B);
    p.g = group_size, p.blocks = ceil_div(K, group_size);
    return run_for_a(p, pl, A, atype, M, K, lda, s, [&](auto out) { return run<decltype(out)::value>(p, pl, bits, s); });
}

}  // extern "C"
