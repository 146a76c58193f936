// The `quant`-domain QDQ functions' product run from the stored integers (include/oq_hip_qdq.h; reference:
// qfunctions/_qdq/qmatmul.py, qfunctions/_qdq/qgemm.py -- DequantizeLinear of the whole weight, then MatMul / Gemm):
//
//       Y[M, N] = A[M, K] . dequant(W) (+ bias)          dequant(W)[k, n] = (q[k, n] - zp[i]) * scale[i]
//             i = 0 (per tensor) | n (per column) | n * (K / g) + k / g (groups of g along K)
//
// The arithmetic, the tile, the split of K, the fp32-A pieces and the epilogue are those of matmul_nbits.hip (nbits_tile.hpp): q - zp is
// an exact 2-byte matrix-core operand, a group's product runs on v_mfma_f32_16x16x32_f16 / _bf16 into an fp32 accumulator and is
// folded into the running sum with the group's fp32 scale by one fma; per tensor / per column the group is the whole of K.  What
// is this file's own is how W reaches LDS: it is one byte per value, [K, N], and its fast axis is n, not k.
//
//   staging   form (b) of the two this tree knows, the register transpose of qlinear_gemm.hip's [K, N] B: a thread loads 8 dwords --
//             4 columns at 8 consecutive k -- with the 32 lanes of a half wave on the 128 consecutive bytes of one k, transposes the
//             two 4 x 4 byte blocks in registers (v_perm_b32), subtracts its columns' zero points and writes 4 x 16 bytes, each 8
//             consecutive k of one column as 2-byte operands, into the [n][k] image the fragments are read from with one 16-byte
//             ds_read -- the image, the fragment reads and the MFMA loop of matmul_nbits.hip.  Form (a), an LDS image that keeps n
//             fast read with ds_read_b64_tr_b16, would need the 2-byte operands made before the transpose (twice the LDS write
//             traffic of the byte transpose's input) and an image whose rows are 8-byte aligned per 4 k; (b) moves bytes, not
//             halves, through the transpose and reuses a layout that is already exact-tested (docs/LAB_NOTES_r29.md).
//   banks     rows are 144 bytes (9 bank quads).  A thread owns columns 4 q + j, and in the order of the columns the 16 lanes that write
//             one j would start in 4 bank quads only; so column 4 q + j lies in row 36 j + q (kColPlane; 140 rows for 128 columns):
//             the rows of neighbouring lanes are neighbours, 16 of them start in 16 different bank quads, and the 16 columns of a
//             fragment read lie in rows 36 j + q0 + q', j, q' = 0 ... 3: 9 (4 j + q') mod 16 covers the 16 bank quads too.
//   rows      where the rows of W are 4-byte aligned (the base is, and ldw % 4 == 0) a thread reads its four columns as one dword;
//             rows of any other alignment, and the last columns of an N that is no multiple of 4, are read byte by byte.
//   signed W  the stored byte is flipped on its way (x ^ 0x80 = q + 128 as an unsigned byte), the zero point likewise: the
//             difference is the same integer, and a missing zero point is the flip of 0.
//   guards    rows >= M and k >= K of A are zeros in LDS.  No byte of W or of its parameters outside [K, N] is read: a thread whose
//             rows run past K or whose columns run past N reads the last row / column again, which meets those zeros of A or
//             lands in outputs that are never stored.
//   body      the kernel below is tile_gemm (nbits_tile.hpp, the body of matmul_nbits.hip's kernels) written out with this file's
//             staging in place.  Built on tile_gemm with the staging as a policy, the fp32-A kernel of the 128-row tile was 0.4 - 3 %
//             slower at M = 2048 in two measurements (docs/LAB_NOTES_r30.md), so this copy stays: a fix to the k loop, the fold
//             or the epilogue is made in both.
// This file is built with -fno-slp-vectorize (_build.py) from its first compile: the fold below is the one that became v_pk_fma_f32
// in matmul_nbits.hip and gave wrong sums on the MI355X (docs/LAB_NOTES_r22.md).
#include "nbits_tile.hpp"

#include "../../include/oq_hip_qdq.h"

namespace oq {
namespace {

constexpr int kColPlane = 36;     // rows of the W image between columns 4 q + j and 4 q + j + 1
constexpr int kRowsW = 3 * kColPlane + kBN / 4;

struct QdqArgs : NbitsArgs {      // B: W;  blocks: the parameters' stride from column to column (0, 1, K / g);  g: beyond K unless grouped
    int64_t ldw;
    uint32_t flip;                // 0x80808080 for a signed W
    int32_t w_vec;                // rows of W are 4-byte aligned
};

template <int OUT, int MT>
__global__ __launch_bounds__(kThreads, OUT == OQ_NBITS_F32 ? 1 : 2) void qdq_gemm_kernel(const QdqArgs p) {
    typedef std::conditional_t<OUT == OQ_NBITS_BF16, OpBF16, OpF16> OP;
    typedef typename OP::frag frag;
    constexpr int PIECES = OUT == OQ_NBITS_F32 ? 2 : 1;
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = PIECES * BM * 8 / kThreads;      // 16-byte chunks of the A tile(s) per thread: PIECES * MT
    __shared__ __attribute__((aligned(16))) unsigned char lds[(PIECES * BM + kRowsW) * kRow];
    unsigned char* const lds_b = lds + PIECES * BM * kRow;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x % p.tiles_m) * BM;
    const int64_t n0 = static_cast<int64_t>(blockIdx.x / p.tiles_m) * kBN;
    const int64_t k_begin = static_cast<int64_t>(blockIdx.y) * p.steps_per_split * kBK;
    const int64_t k_end = min(p.K, k_begin + p.steps_per_split * kBK);
    const uint32_t g32 = static_cast<uint32_t>(p.g);      // k < 2^31 and g <= 2^31 (kOneGroup): the group of a k is a 32-bit quotient

    // what this thread stages: A_CHUNKS chunks of A, and of W the columns kn_n ... + 3 at k = 8 kn_kb ... + 7 of the step
    u32x4 a_regs[A_CHUNKS];
    uint32_t b_regs[8];
    uint32_t zp_raw = 0;      // the four columns' zero points of the staged group, a byte each
    const int kn_nb = tid & 31, kn_kb = tid >> 5;
    const int64_t kn_n = n0 + 4 * kn_nb;
    const bool kn_vec = p.w_vec != 0 && kn_n + 4 <= p.N;      // n0 + 4 kn_nb keeps the alignment of the rows

    auto load_step = [&](int64_t k) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            const int piece = id / (BM * 8), r = (id >> 3) % BM, kc = id & 7;
            const int64_t m = m0 + r;
            const uint16_t* base = (PIECES == 2 && piece == 1) ? p.A_lo : p.A;
            a_regs[i] = (m < p.M && k + kc * 8 < p.Ka) ? load_a8(base + m * p.lda, k + kc * 8, p.Ka, p.a_vec != 0) : u32x4{0u, 0u, 0u, 0u};
        }
        // Nothing below is guarded load by load: a row past K repeats row K - 1 and a column past N column N - 1.  Both meet zeros
        // of A or belong to outputs that are never stored, and every byte is a finite integer.
        const int64_t kk = k + 8 * kn_kb;
#pragma unroll
        for (int i = 0; i < 8; ++i) b_regs[i] = 0u;
        if (kk < k_end && kn_n < p.N) {
            const uint8_t* src = p.B + kk * p.ldw + kn_n;
            if (kn_vec) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    b_regs[i] = *reinterpret_cast<const uint32_t*>(src);
                    if (kk + i + 1 < p.K) src += p.ldw;
                }
            } else {
                const int last = static_cast<int>(min(static_cast<int64_t>(3), p.N - 1 - kn_n));
                const int o1 = min(1, last), o2 = min(2, last);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    b_regs[i] = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[o1]) << 8) | (static_cast<uint32_t>(src[o2]) << 16) |
                                (static_cast<uint32_t>(src[last]) << 24);
                    if (kk + i + 1 < p.K) src += p.ldw;
                }
            }
        }
        if (p.blocks <= 1 && k != k_begin) return;      // per tensor / per column: the zero points of the first step are those of every step
        zp_raw = 0u;
        if (p.zp != nullptr && kk < k_end && kn_n < p.N) {
            // g is a multiple of 32 and k of 64: the group of kk is that of k or of k + 32, two uniform quotients (of 32 bits: k < 2^31)
            const uint32_t kb_lo = static_cast<uint32_t>(k) / g32, kb_hi = static_cast<uint32_t>(k + 32) / g32;
            const int64_t kb = kn_kb >= 4 ? kb_hi : kb_lo;
            const uint8_t* z = p.zp + kn_n * p.blocks + kb;      // walks the four columns and stays on the last one that exists
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                zp_raw |= static_cast<uint32_t>(*z) << (8 * j);
                if (kn_n + j + 1 < p.N) z += p.blocks;
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            *reinterpret_cast<u32x4*>(lds + (id >> 3) * kRow + (id & 7) * 16) = a_regs[i];      // id >> 3 = piece * BM + r
        }
        uint32_t c[2][4];      // r[j]: columns n .. n + 3 at k + j  ->  c[j]: k .. k + 3 of column n + j
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t r0 = b_regs[4 * i] ^ p.flip, r1 = b_regs[4 * i + 1] ^ p.flip, r2 = b_regs[4 * i + 2] ^ p.flip, r3 = b_regs[4 * i + 3] ^ p.flip;
            const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
            const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
            c[i][0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[i][1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
            c[i][2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[i][3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
        }
        const uint32_t zp_flipped = zp_raw ^ p.flip;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float zpf = static_cast<float>((zp_flipped >> (8 * j)) & 0xFFu);
            uint32_t d[4];
            dequant_word<OP, 8>(c[0][j], zpf, d);
            dequant_word<OP, 8>(c[1][j], zpf, d + 2);
            *reinterpret_cast<u32x4*>(lds_b + (kColPlane * j + kn_nb) * kRow + 16 * kn_kb) = u32x4{d[0], d[1], d[2], d[3]};
        }
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
    int64_t in_group = static_cast<uint32_t>(k_begin) % g32;      // k of the next MFMA depth inside its group
    if (k_begin < k_end) load_scales(static_cast<uint32_t>(k_begin) / g32, sc);

    const unsigned char* const a_frag = lds + (wm * 16 * MT + (lane & 15)) * kRow + (lane >> 4) * 16;
    const unsigned char* const b_frag = lds_b + (kColPlane * (lane & 3) + wn * 16 + ((lane & 15) >> 2)) * kRow + (lane >> 4) * 16;      // + 4 nt rows

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
                for (int nt = 0; nt < NT; ++nt) b[nt] = __builtin_bit_cast(frag, *reinterpret_cast<const u32x4*>(b_frag + nt * 4 * kRow + s * 64));
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
                    if (ks + 32 < k_end) load_scales(static_cast<uint32_t>(ks + 32) / g32, sc);
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
constexpr NbitsRoute kRoute{"oq_qdq_matmul", kMaxExtent, 32, "two groups would share one 32-deep matrix instruction", false};
constexpr int64_t kOneGroup = 1LL << 31;      // g of a per-tensor / per-column call: no k reaches it, the fold happens at the end of K

template <int OUT>
int32_t run(const QdqArgs& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { qdq_gemm_kernel<OUT, decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
    const int32_t st = check_launch("qdq_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    return reduce_slabs<OUT>(p, pl, s);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_extension_version(void) { return OQ_QDQ_EXTENSION_VERSION; }

size_t oq_qdq_matmul_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t atype) {
    return plan_workspace_bytes(M, K, N, K, atype, [&] {
        set_error("oq_qdq_matmul_workspace_bytes: M=%lld K=%lld N=%lld atype=%d outside the bounds", (long long)M, (long long)K, (long long)N, atype);
    });
}

int32_t oq_qdq_matmul(const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, const void* W, int32_t wtype, int64_t N, int64_t ldw,
                      int32_t granularity, int64_t group_size, const void* scales, int32_t scales_type, const void* zero_points, const void* bias,
                      void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = kRoute.fn;
    int32_t st = operands_ok(fn, A, W, scales, Y, atype, scales_type);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(wtype == OQ_UINT8 || wtype == OQ_INT8, OQ_ERR_INVALID_ARGUMENT, "%s: unknown wtype %d (OQ_UINT8 and OQ_INT8: one byte per value)", fn, wtype);
    OQ_REQUIRE(granularity == OQ_TENSOR || granularity == OQ_CHANNEL || granularity == OQ_GROUP, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown granularity %d", fn, granularity);
    const bool grouped = granularity == OQ_GROUP;
    st = extents_and_flags_ok(kRoute, M, K, N, lda, ldy, 8, grouped ? group_size : kRoute.group_unit, 0);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(matrix_ok(K, N, ldw), OQ_ERR_INVALID_ARGUMENT, "%s: K=%lld N=%lld ldw=%lld outside the bounds", fn, (long long)K, (long long)N,
               (long long)ldw);
    OQ_REQUIRE(!grouped || K % group_size == 0, OQ_ERR_UNSUPPORTED, "%s: K = %lld is no multiple of group_size = %lld (a [K, N] matrix has no padded group)",
               fn, (long long)K, (long long)group_size);
    OQ_REQUIRE(tile_shape_ok(M, K, N, K), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld: an operand beyond 2^40 elements", fn, (long long)M,
               (long long)K, (long long)N);
    st = element_alignment_ok(fn, A, Y, bias, scales, atype, scales_type);
    if (st != OQ_OK) return st;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const Plan pl = make_plan(M, K, N, atype, ws);
    st = workspace_ok(fn, ws, workspace, workspace_bytes);
    if (st != OQ_OK) return st;

    hipStream_t s = as_stream(stream);
    QdqArgs p{};
    fill_args(p, scales, scales_type, zero_points, bias, Y, ldy, M, N, K, pl);
    p.B = static_cast<const uint8_t*>(W);
    p.ldw = ldw;
    p.flip = wtype == OQ_INT8 ? 0x80808080u : 0u;
    p.w_vec = aligned_to(W, 4) && ldw % 4 == 0;
    p.g = grouped ? group_size : kOneGroup;
    p.blocks = grouped ? K / group_size : granularity == OQ_CHANNEL ? 1 : 0;
    return run_for_a(p, pl, A, atype, M, K, lda, s, [&](auto out) { return run<decltype(out)::value>(p, pl, s); });
}

}  // extern "C"
