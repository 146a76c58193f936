// The `quant`-domain QDQ functions' product run from a 4-bit weight as the file stores it (include/oq_hip_qdq_packed4.h, DESIGN.md
// 4.32): an ONNX INT4 / UINT4 initializer [K, N], two values a byte in flat order, the even index in the low nibble -- what
// OQ_LAYOUT_KN_PACKED4 (oq_hip.h) writes on the quantize side.  With an even N every row starts on a byte: a [K, N / 2] byte matrix.
//
//       Y[M, N] = A[M, K] . dequant(W) (+ bias)          dequant(W)[k, n] = (q[k, n] - zp[i]) * scale[i]
//             q[k, n] = nibble (n & 1) of byte W[k * ldw + n / 2]          i as in oq_qdq_matmul (qdq_matmul.hip)
//
// The arithmetic is that of oq_qdq_matmul: q - zp, here in [-15, 15], is an exact 2-byte matrix-core operand, a group's product runs
// on v_mfma_f32_16x16x32_f16 / _bf16 into an fp32 accumulator and is folded into the running sum with the group's fp32 scale by one
// fma.  The kernel is tile_gemm (nbits_tile.hpp) with this file's staging policy, Packed4Stage: the [n][k] image of 2-byte operands,
// the 16-byte fragment reads, the MFMA loop, the fold, the epilogue, the plan, the split of K and its reduce kernel are that
// header's text.  What is this file's own is how W reaches LDS.
//
//   staging   a 64-k x 128-column step is 64 rows of 64 bytes: 4 dwords for each of the 256 threads (the byte route loads 8).  Thread
//             t owns the dword cb = t & 15 of a row -- the 8 neighbouring columns 8 cb ... 8 cb + 7 -- at the 4 consecutive
//             k = 4 kq ... 4 kq + 3, kq = t >> 4: the 16 lanes of a quarter wave lie on the 64 consecutive bytes of one row, the 16
//             quarter waves of the block cover the 64 k.  A loaded dword d splits into d & 0x0F0F0F0F, the four even columns as
//             bytes, and (d >> 4) & 0x0F0F0F0F, the four odd ones.  Each of the two 4 x 4 byte blocks (4 columns x 4 k) is
//             transposed in registers with the v_perm_b32 network of qdq_matmul.hip, which leaves the 4 consecutive k of one column
//             in a dword; that dword minus the column's zero point is two dwords of operands (dequant_word), written as 8 bytes at
//             byte 8 kq of the column's image row.  8 writes of 8 bytes per thread and step.
//   banks     rows are 144 bytes: 18 bank pairs, 9 bank quads.  Column 8 cb + c lies in image row 18 c + cb (kColPlane = 18; 142
//             rows for 128 columns), so the rows of neighbouring lanes are neighbours.
//             writes: one write instruction has c fixed.  The 32 lanes of a half wave are cb = 0 ... 15 at kq0 and kq0 + 1, kq0
//             even; their 8 bytes start in bank pair 18 (18 c + cb) + kq mod 32.  18 cb mod 32 takes the 16 even residues once
//             each, kq0 keeps them even, kq0 + 1 makes them odd: 32 lanes, 32 different bank pairs.
//             reads: the 16 columns of the fragment nt of column half wn are 64 wn + 16 nt + l, l = lane & 15: cb = 8 wn + 2 nt +
//             (l >> 3), c = l & 7, so the row is 18 (l & 7) + (l >> 3) + 8 wn + 2 nt (frag_row; kFragStride = 2).  Their 16 bytes
//             start in bank quad 9 row mod 16; 9 is a unit mod 16 and 18 c + h = 2 c + h mod 16, c = 0 ... 7, h = 0, 1, takes all
//             16 residues: 16 lanes, 16 different bank quads, as in the images of matmul_nbits.hip and qdq_matmul.hip.
//   rows      where the rows of W are 4-byte aligned (the base is, and ldw % 4 == 0) a thread reads its 8 columns as one dword
//             (n0 / 2 + 4 cb keeps the alignment); rows of any other alignment, and the last columns of an N that is no multiple of
//             8, are read byte by byte.
//   signed W  every nibble is flipped on its way (x ^ 8 = q + 8 as an unsigned nibble), the zero point likewise: the difference is
//             the same integer, and a missing zero point is the flip of 0.  Zero points are one value per byte in the container
//             type, inside the 4-bit range; the low nibble of the flipped byte is what is subtracted.
//   guards    rows >= M and k >= K of A are zeros in LDS.  No byte outside [K, N / 2] of W, and no parameter outside its tensor, is
//             read: a thread whose k run past K or whose columns run past N reads the last row / byte / column again, which meets
//             those zeros of A or lands in outputs that are never stored, and every nibble is a finite integer.  No load is guarded on
//             its own.  Zero points are loaded once per tensor / per column (the first step's are every step's); per group they
//             are loaded per step, from one of two wave-uniform quotients: g is a multiple of 32 and k of 64, so the group of a
//             thread's k is that of k (kq < 8) or of k + 32.
//   odd N     is refused by name: in the flat packing the rows of an odd N start on alternating nibbles.
// Built with -fno-slp-vectorize (_build.py) from its first compile, like every file that holds tile_gemm's fold (docs/LAB_NOTES_r22.md).
#include "nbits_tile.hpp"

#include "../../include/oq_hip_qdq_packed4.h"

namespace oq {
namespace {

constexpr int kColPlane = 18;     // rows of the W image between columns 8 cb + c and 8 cb + c + 1

struct Packed4Args : NbitsArgs {      // B: W;  blocks: the parameters' stride from column to column (0, 1, K / g);  g: beyond K unless grouped
    int64_t ldw;                      // bytes
    uint32_t flip;                    // 0x88888888 for a signed W
    int32_t w_vec;                    // rows of W are 4-byte aligned
};

// r[i]: bytes of columns j = 0 ... 3 at k + i  ->  c[j]: bytes of k ... k + 3 of column j
__device__ __forceinline__ void transpose4x4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&c)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
    const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

struct Packed4Stage {
    typedef Packed4Args args;
    static constexpr int kRows = 7 * kColPlane + kBN / 8, kFragStride = 2;
    static constexpr bool kFloatZp = false;
    static __device__ __forceinline__ int frag_row(int wn, int lane) { return kColPlane * (lane & 7) + ((lane & 15) >> 3) + 8 * wn; }
    // k < 2^31 and g <= 2^31 (kOneGroup): the group of a k is a 32-bit quotient
    static __device__ __forceinline__ int64_t group(const Packed4Args& p, int64_t k) { return static_cast<uint32_t>(k) / static_cast<uint32_t>(p.g); }
    static __device__ __forceinline__ int64_t within(const Packed4Args& p, int64_t k) { return static_cast<uint32_t>(k) % static_cast<uint32_t>(p.g); }

    uint32_t b_regs[4];           // columns pn ... pn + 7 at k = 4 kq + i of the step
    uint32_t zp_raw[2] = {0, 0};  // the eight columns' zero points of the staged group, a byte each
    const int cb, kq;
    const int64_t pn;             // the thread's first column
    const bool vec;

    __device__ __forceinline__ Packed4Stage(const Packed4Args& p, int tid, int64_t n0)
        : cb(tid & 15), kq(tid >> 4), pn(n0 + 8 * cb), vec(p.w_vec != 0 && pn + 8 <= p.N) {}

    __device__ __forceinline__ void load(const Packed4Args& p, int64_t k, int64_t k_begin, int64_t k_end) {
        // Nothing below is guarded load by load: a row past K repeats row K - 1, a byte past N / 2 byte N / 2 - 1 and a column past N
        // column N - 1.  All meet zeros of A or belong to outputs that are never stored.
        const int64_t kk = k + 4 * kq;
#pragma unroll
        for (int i = 0; i < 4; ++i) b_regs[i] = 0u;
        if (kk < k_end && pn < p.N) {
            const uint8_t* src = p.B + kk * p.ldw + (pn >> 1);
            if (vec) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b_regs[i] = *reinterpret_cast<const uint32_t*>(src);
                    if (kk + i + 1 < p.K) src += p.ldw;
                }
            } else {
                const int last = static_cast<int>(min(static_cast<int64_t>(3), ((p.N - pn) >> 1) - 1));      // N is even: >= 0
                const int o1 = min(1, last), o2 = min(2, last);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b_regs[i] = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[o1]) << 8) | (static_cast<uint32_t>(src[o2]) << 16) |
                                (static_cast<uint32_t>(src[last]) << 24);
                    if (kk + i + 1 < p.K) src += p.ldw;
                }
            }
        }
        if (p.blocks <= 1 && k != k_begin) return;      // per tensor / per column: the zero points of the first step are those of every step
        zp_raw[0] = zp_raw[1] = 0u;
        if (p.zp != nullptr && kk < k_end && pn < p.N) {
            const uint32_t g32 = static_cast<uint32_t>(p.g);
            const uint32_t kb_lo = static_cast<uint32_t>(k) / g32, kb_hi = static_cast<uint32_t>(k + 32) / g32;
            const int64_t kb = kq >= 8 ? kb_hi : kb_lo;
            const uint8_t* z = p.zp + pn * p.blocks + kb;      // walks the eight columns and stays on the last one that exists
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                zp_raw[c >> 2] |= static_cast<uint32_t>(*z) << (8 * (c & 3));
                if (pn + c + 1 < p.N) z += p.blocks;
            }
        }
    }

    template <typename OP>
    __device__ __forceinline__ void store(const Packed4Args& p, unsigned char* lds_b) const {
        uint32_t even[4], odd[4];      // even[j]: k ... k + 3 of column pn + 2 j;  odd[j]: of column pn + 2 j + 1
        {
            const uint32_t r0 = b_regs[0] ^ p.flip, r1 = b_regs[1] ^ p.flip, r2 = b_regs[2] ^ p.flip, r3 = b_regs[3] ^ p.flip;
            transpose4x4(r0 & 0x0F0F0F0Fu, r1 & 0x0F0F0F0Fu, r2 & 0x0F0F0F0Fu, r3 & 0x0F0F0F0Fu, even);
            transpose4x4((r0 >> 4) & 0x0F0F0F0Fu, (r1 >> 4) & 0x0F0F0F0Fu, (r2 >> 4) & 0x0F0F0F0Fu, (r3 >> 4) & 0x0F0F0F0Fu, odd);
        }
        const uint32_t zp_flipped[2] = {(zp_raw[0] ^ p.flip) & 0x0F0F0F0Fu, (zp_raw[1] ^ p.flip) & 0x0F0F0F0Fu};
        unsigned char* const dst = lds_b + cb * kRow + 8 * kq;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float zpf = static_cast<float>((zp_flipped[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            uint32_t d[2];
            dequant_word<OP, 8>(c & 1 ? odd[c >> 1] : even[c >> 1], zpf, d);
            *reinterpret_cast<u32x2*>(dst + kColPlane * c * kRow) = u32x2{d[0], d[1]};
        }
    }
};

// The launch bounds of nbits_gemm_kernel (matmul_nbits.hip says why): two waves per SIMD for a 2-byte A, one for the two pieces of an fp32 A.
template <int OUT, int MT>
__global__ __launch_bounds__(kThreads, OUT == OQ_NBITS_F32 ? 1 : 2) void qdq_packed4_gemm_kernel(const Packed4Args p) { tile_gemm<OUT, MT, Packed4Stage>(p); }

// ---- host
constexpr NbitsRoute kRoute{"oq_qdq_matmul_packed4", kMaxExtent, 32, "two groups would share one 32-deep matrix instruction", false};
constexpr int64_t kOneGroup = 1LL << 31;      // g of a per-tensor / per-column call: no k reaches it, the fold happens at the end of K

template <int OUT>
int32_t run(const Packed4Args& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { qdq_packed4_gemm_kernel<OUT, decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
    const int32_t st = check_launch("qdq_packed4_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    return reduce_slabs<OUT>(p, pl, s);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_packed4_extension_version(void) { return OQ_QDQ_PACKED4_EXTENSION_VERSION; }

size_t oq_qdq_matmul_packed4_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t atype) {
    return plan_workspace_bytes(M, K, N, K, atype, [&] {
        set_error("oq_qdq_matmul_packed4_workspace_bytes: M=%lld K=%lld N=%lld atype=%d outside the bounds", (long long)M, (long long)K, (long long)N,
                  atype);
    });
}

int32_t oq_qdq_matmul_packed4(const void* A, int32_t atype, int64_t M, int64_t K, int64_t lda, const void* W, int32_t wtype, int64_t N, int64_t ldw,
                              int32_t granularity, int64_t group_size, const void* scales, int32_t scales_type, const void* zero_points,
                              const void* bias, void* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = kRoute.fn;
    int32_t st = operands_ok(fn, A, W, scales, Y, atype, scales_type);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(wtype == OQ_UINT4 || wtype == OQ_INT4, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown wtype %d (OQ_UINT4 and OQ_INT4: two values per byte; oq_qdq_matmul takes one value per byte)", fn, wtype);
    OQ_REQUIRE(granularity == OQ_TENSOR || granularity == OQ_CHANNEL || granularity == OQ_GROUP, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown granularity %d", fn, granularity);
    const bool grouped = granularity == OQ_GROUP;
    st = extents_and_flags_ok(kRoute, M, K, N, lda, ldy, 4, grouped ? group_size : kRoute.group_unit, 0);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(N % 2 == 0, OQ_ERR_UNSUPPORTED, "%s: N = %lld is odd (the rows of a flat-packed [K, N] start on alternating nibbles: no byte matrix)", fn,
               (long long)N);
    OQ_REQUIRE(matrix_ok(K, N / 2, ldw), OQ_ERR_INVALID_ARGUMENT, "%s: K=%lld N=%lld ldw=%lld outside the bounds (ldw counts bytes, >= N / 2)", fn,
               (long long)K, (long long)N, (long long)ldw);
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
    Packed4Args p{};
    fill_args(p, scales, scales_type, zero_points, bias, Y, ldy, M, N, K, pl);
    p.B = static_cast<const uint8_t*>(W);
    p.ldw = ldw;
    p.flip = wtype == OQ_INT4 ? 0x88888888u : 0u;
    p.w_vec = aligned_to(W, 4) && ldw % 4 == 0;
    p.g = grouped ? group_size : kOneGroup;
    p.blocks = grouped ? K / group_size : granularity == OQ_CHANNEL ? 1 : 0;
    return run_for_a(p, pl, A, atype, M, K, lda, s, [&](auto out) { return run<decltype(out)::value>(p, pl, s); });
}

}  // extern "C"
