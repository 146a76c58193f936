// com.microsoft::MatMulNBits run from the packed blob (include/oq_hip_nbits.h):
//
//       Y[M, N] = A[M, K] . dequant(B)^T (+ bias)          dequant(B)[n, k] = (q[n, k] - zp[n, k / g]) * scale[n, k / g]
//
// q - zp is an integer in [-255, 255] and so exact in fp16 and bf16: per k-group the product A_g . (q - zp)_g runs on
// v_mfma_f32_16x16x32_f16 / _bf16 with an exact B operand into an fp32 accumulator, which is then folded into the running sum with the
// group's fp32 scale (one fma per group and output element).  The [N, K] weight never exists, in memory or in LDS: a workgroup
// dequantizes the 128 x 64 integers of its current k-step into LDS, as 2-byte operands, and nothing else.
//
//   block     256 threads = 2 x 2 waves; tile 32 * MT rows (MT = 4: 128; MT = 1: 32, for M <= 32) x 128 columns; k-step 64.
//   wave      16 * MT x 64 outputs = MT x 4 MFMA tiles; per tile 4 fp32 of the group accumulator and 4 of the running sum.
//   operands  both have k as their fast axis in memory, which is what the 16x16x32 lane map wants (lane l: row / column l & 15,
//             k = 8 (l >> 4) ... + 7): a 16-byte ds_read per fragment, rows padded to 144 bytes (conflict-free).
//   staging   registers: the global loads of step i + 1 are issued before the MFMAs of step i; one LDS buffer, two barriers a step.
//   fp32 A    nbits_split_rows_kernel writes two fp16 pieces per element under one power-of-two scale per row (the row's largest
//             lands in [2^14, 2^15)): hi = fp16(x s), lo = fp16((x s - hi) 2^11).  lo meets B 2^-11 (exact: |q - zp| >= 1 keeps
//             it a normal fp16), so both products share the accumulator.  A hi that would be an fp16 subnormal is dropped into lo.
//   split K   few output tiles (small M): blockIdx.y takes a range of k-steps, writes its sum to slab y; nbits_reduce_kernel adds
//             the slabs in slab order and finishes.  No atomics anywhere.
//   guards    every global access is guarded by M, N, K: rows >= M, columns >= N and k >= K are zeros in LDS (A) or never read
//             (B, scales, zero points); a padded blob position meets a zero of A and its bytes are finite integers whatever they hold.
// The matrix-core operand, the decoders of the blob and of a packed zero point, and the checks of a call are those of the decode
// route too: nbits_common.hpp.  The argument block, the rounding, the reduce and split-rows kernels, the plan and its workspace are
// those of the [K, N] byte-matrix GEMM too (qdq_matmul.hip): nbits_tile.hpp, whose make_plan lays the workspace out around
// make_tile_plan(M, K, N).
#include "nbits_tile.hpp"
#include "tile_plan.hpp"

namespace oq {
namespace {

// 32 stored values (k ascending) minus the zero point -> 32 exact 2-byte operands
template <typename OP, int BITS>
__device__ __forceinline__ void dequant32(const u32x4 (&raw)[BITS / 4], float zpf, u32x4 (&out)[4]) {
    uint32_t d[16];
#pragma unroll
    for (int wi = 0; wi < BITS; ++wi) dequant_word<OP, BITS>(raw[wi >> 2][wi & 3], zpf, d + wi * (16 / BITS));
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = u32x4{d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]};
}

// Two waves per SIMD (<= 256 registers, no scratch) for a 2-byte A: unbounded, the 128-row tile takes 230 VGPRs + 64 AGPRs, one wave
// per SIMD, and runs at less than half the speed (0.92 against 0.42 ms at 2048 x 4096 x 11008).  The fp32-A kernels stage two A pieces
// and keep one wave per SIMD (the 8-bit one needs scratch under the bound).
// This file is built with -fno-slp-vectorize (_build.py): paired, the fold below becomes v_pk_fma_f32 with an op_sel on the scale
// pair, which on the MI355X gave wrong low halves in lanes 48 .. 63 whenever several waves shared a SIMD (docs/LAB_NOTES_r22.md).
template <int OUT, int BITS, int MT>
__global__ __launch_bounds__(kThreads, OUT == OQ_NBITS_F32 ? 1 : 2) void nbits_gemm_kernel(const NbitsArgs p) {
    typedef std::conditional_t<OUT == OQ_NBITS_BF16, OpBF16, OpF16> OP;
    typedef typename OP::frag frag;
    constexpr int PIECES = OUT == OQ_NBITS_F32 ? 2 : 1;
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = PIECES * BM * 8 / kThreads;      // 16-byte chunks of the A tile(s) per thread: PIECES * MT
    __shared__ __attribute__((aligned(16))) unsigned char lds[(PIECES * BM + kBN) * kRow];
    unsigned char* const lds_b = lds + PIECES * BM * kRow;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x % p.tiles_m) * BM;
    const int64_t n0 = static_cast<int64_t>(blockIdx.x / p.tiles_m) * kBN;
    const int64_t k_begin = static_cast<int64_t>(blockIdx.y) * p.steps_per_split * kBK;
    const int64_t k_end = min(p.K, k_begin + p.steps_per_split * kBK);

    // what this thread stages: A_CHUNKS chunks of A, and 32 values of one row of B
    u32x4 a_regs[A_CHUNKS];
    u32x4 b_regs[BITS / 4];
    uint32_t zp_raw = 0;      // the staged group's zero point, converted where it is used: no wait for it in front of the MFMAs
    const int b_row = tid >> 1, b_half = tid & 1;
    const int64_t b_n = n0 + b_row;

    auto load_step = [&](int64_t k) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            const int piece = id / (BM * 8), r = (id >> 3) % BM, kc = id & 7;
            const int64_t m = m0 + r;
            const uint16_t* base = (PIECES == 2 && piece == 1) ? p.A_lo : p.A;
            a_regs[i] = (m < p.M && k + kc * 8 < p.Ka) ? load_a8(base + m * p.lda, k + kc * 8, p.Ka, p.a_vec != 0) : u32x4{0u, 0u, 0u, 0u};
        }
        const int64_t kb_k = k + 32 * b_half;
#pragma unroll
        for (int i = 0; i < BITS / 4; ++i) b_regs[i] = u32x4{0u, 0u, 0u, 0u};
        zp_raw = 1u << (BITS - 1);
        if (b_n < p.N && kb_k < k_end) {
            const int64_t kb = kb_k / p.g, within = kb_k - kb * p.g;
            const uint8_t* src = p.B + ((b_n * p.blocks + kb) * p.g + within) * BITS / 8;
#pragma unroll
            for (int i = 0; i < BITS / 4; ++i) b_regs[i] = reinterpret_cast<const u32x4*>(src)[i];
            if (p.zp != nullptr) {
                zp_raw = zp_byte<BITS>(p.zp, b_n, p.blocks, kb);      // shifted here, masked where it is used (store_step), not by zp_of_byte
                if constexpr (BITS == 4) zp_raw >>= 4 * (kb & 1);
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            *reinterpret_cast<u32x4*>(lds + (id >> 3) * kRow + (id & 7) * 16) = a_regs[i];      // id >> 3 = piece * BM + r
        }
        u32x4 d[4];
        dequant32<OP, BITS>(b_regs, static_cast<float>(zp_raw & ((1u << BITS) - 1)), d);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(lds_b + b_row * kRow + b_half * 64 + i * 16) = d[i];
    };

    f32x4 sum[MT][NT], acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sum[mt][nt] = acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int64_t col = n0 + wn * 64 + (lane & 15);          // + 16 nt: the output column of this lane in tile nt
    auto load_scales = [&](int64_t kb, float (&sc)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t n = col + 16 * nt;
            sc[nt] = 0.0f;
            if (n < p.N) sc[nt] = p.scales_f32 ? static_cast<const float*>(p.scales)[n * p.blocks + kb] : OP::one(static_cast<const uint16_t*>(p.scales)[n * p.blocks + kb]);
        }
    };
    float sc[NT];
    int64_t in_group = k_begin % p.g;      // k of the next MFMA depth inside its group
    if (k_begin < k_end) load_scales(k_begin / p.g, sc);

    const unsigned char* const a_frag = lds + (wm * 16 * MT + (lane & 15)) * kRow + (lane >> 4) * 16;
    const unsigned char* const b_frag = lds_b + (wn * 64 + (lane & 15)) * kRow + (lane >> 4) * 16;

    if (k_begin < k_end) load_step(k_begin);
    for (int64_t k = k_begin; k < k_end; k += kBK) {
        store_step();
        __syncthreads();
        if (k + kBK < k_end) load_step(k + kBK);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t ks = k + 32 * s;
            if (ks < k_end) {
                frag b[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b[nt] = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(b_frag + nt * 16 * kRow + s * 64));
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const frag a = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(a_frag + mt * 16 * kRow + s * 64));
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = OP::mma(a, b[nt], acc[mt][nt]);
                }
                if constexpr (PIECES == 2) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b[nt] = b[nt] * static_cast<_Float16>(0.00048828125f);      // 2^-11, exact
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const frag a = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(a_frag + (BM + mt * 16) * kRow + s * 64));
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = OP::mma(a, b[nt], acc[mt][nt]);
                    }
                }
                in_group += 32;
                if (in_group == p.g || ks + 32 >= k_end) {      // the group (or this block's part of it) is complete
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) sum[mt][nt][r] = __builtin_fmaf(acc[mt][nt][r], sc[nt], sum[mt][nt][r]);
                            acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                        }
                    in_group = 0;
                    if (ks + 32 < k_end) load_scales((ks + 32) / p.g, sc);
                }
            }
        }
        __syncthreads();
    }

    // C/D map of the 16x16 MFMAs: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wm * 16 * MT + mt * 16 + 4 * (lane >> 4) + r, n = col + 16 * nt;
                if (m < p.M && n < p.N) {
                    if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = sum[mt][nt][r];
                    else finish<OUT>(p, m, n, sum[mt][nt][r]);
                }
            }
}

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
    if (!type_ok(atype) || !tile_shape_ok(M, K, N, group_size)) {
        set_error("oq_matmul_nbits_workspace_bytes: M=%lld K=%lld N=%lld group_size=%lld atype=%d outside the bounds", (long long)M, (long long)K,
                  (long long)N, (long long)group_size, atype);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, atype, ws);
    return ws.total();
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
    p.B = static_cast<const uint8_t*>(B);
    p.scales = scales;
    p.scales_f32 = scales_type == OQ_NBITS_F32;
    p.zp = zero_points;
    p.bias = bias;
    p.Y = Y;
    p.ldy = ldy;
    p.M = M, p.N = N, p.K = K, p.g = group_size, p.blocks = ceil_div(K, group_size);
    p.tiles_m = pl.tiles_m, p.steps_per_split = pl.steps_per_split;
    p.slab = pl.slab;
    if (atype == OQ_NBITS_F32) {
        st = split_rows(p, pl, A, M, K, lda, s);
        if (st != OQ_OK) return st;
        return run<OQ_NBITS_F32>(p, pl, bits, s);
    }
    p.A = static_cast<const uint16_t*>(A), p.lda = lda, p.Ka = K, p.a_vec = aligned_to(A, 16) && lda % 8 == 0;
    return atype == OQ_NBITS_BF16 ? run<OQ_NBITS_BF16>(p, pl, bits, s) : run<OQ_NBITS_F16>(p, pl, bits, s);
}

}  // extern "C"
