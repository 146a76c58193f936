// The decode route of a `quant`-domain QDQ function with quantized activations on a 4-bit weight held as packed nibbles
// (include/oq_hip_qdq_function_packed4_decode.h): the call of qdq_function_packed4.hip for 1 ... 16 rows of X.  W --
// [K, N / 2] bytes, value [k, 2 j] in the low nibble of byte [k, j] -- is read once, from global memory straight into the registers
// that feed v_mfma_i32_16x16x64_i8.
//
//       q_x[m, k] = the static quantizer, or DynamicQuantizeLinear's with the parameters of X          quant_k16, qlinear_epilogue.hpp
//       B[k, n]   = W[k, n] - zp_w[n]                       an int8 in [-15, 15], formed in registers
//       S[m, n]   = sum_k (q_x[m, k] - 128 [uint8]) * B[k, n] - zp_x' * sum_k B[k, n]                  exact, uint32 arithmetic
//       Y         = finish_qdq on S, with B signed and without a zero point: the epilogue text of qdq_function_packed4.hip
//
//   split     grid (ceil(N / 128), splits): a workgroup takes 128 columns and one slice of K (the plan:
//             qdq_function_packed4_decode_plan.hpp), its four waves a quarter of the slice each, in spans of 64 k.
//   A         the workgroup quantizes its slice of X into LDS as [16][slice + kPad] int8, flipped (x ^ 0x80 for uint8) on the way in;
//             rows >= M are zeros.  kPad = 80: a row is an odd number of 16-byte bank quads, so the 16 rows a 16-lane group reads
//             lie in 16 different quads, and a wave whose quarter is no whole span may read up to 48 bytes past the slice inside
//             the row -- whatever lies there meets a zero of B.  One 16-byte LDS read per span is the lane's A fragment: lane & 15
//             the row, lane >> 4 the 16-k chunk.
//   B         lane l: group g = l >> 4, column slot c = l & 15.  Per span the lane loads the dword c of the wave's column block -- the
//             columns 8 c ... 8 c + 7 -- of the 16 rows 64 s + 16 g ... + 15: a 16-lane group lies on 64 contiguous bytes of a row.
//             A dword d, flipped nibble by nibble for a signed W, splits into d & 0x0F0F0F0F (the even columns as bytes) and
//             (d >> 4) & 0x0F0F0F0F (the odd ones); the zero points are subtracted byte by byte and four dwords at a time go
//             through the v_perm_b32 4 x 4 byte transpose (the text of qdq_function_packed4.hip).  Four transposes give, for one
//             column, the 16 consecutive k of the lane's rows as four dwords: the lane's share of the matrix instruction's B operand
//             (column index lane & 15, k chunk lane >> 4).  So MFMA number j of a span multiplies the 16 columns {8 c + j}; its
//             result column lane & 15 is column 8 (lane & 15) + j of the block: an index in the epilogue.
//   pipeline  the 16 loads of span s + 1 are issued before the arithmetic of span s; nothing is consumed where it is loaded.
//   sums      SUMS: one more MFMA per operand against a fragment of ones: row 0 of its result is sum_k B[k, n] over the wave's k.
//   guards    a row k at or beyond the wave's end takes no load: its dword is the packed zero points themselves, so B is exactly 0
//             there, in the product and in the sums.  A lane whose columns lie at or beyond N loads nothing.  A last dword that
//             is partly beyond N / 2 bytes, and every dword of rows that are not 4-byte aligned, is read byte by byte, the last
//             byte that exists again for those that do not (columns that are never stored).
//   fold      the waves leave their 16 x 128 int32 sums (and the column sums) in LDS, which the A slice no longer needs; thread t then
//             adds the four of column t & 127 for the rows t >> 7, + 2, ..., corrects by zp_x' * the column sum and writes the slab
//             (splits > 1: qq_reduce_kernel of qdq_function_parts.hpp adds the slabs and finishes) or finishes through finish_qdq.
// Built with the packed fp32 instructions switched off (_build.py), like qdq_function_packed4.hip: the same epilogue, the same bytes.
#include "qdq_function_parts.hpp"
#include "qdq_function_packed4_decode_plan.hpp"

#include "../../include/oq_hip_qdq_function_packed4_decode.h"

namespace oq {
namespace {

constexpr int64_t kMaxK = 561433;     // 255 * 15 * K <= 2^31 - 1: no int32 sum can wrap
constexpr int kPad = 80;              // bytes behind a row of the A slice in LDS
constexpr int kFoldWords = kWaves * 16 * kP4DecodeCols;                  // the waves' sums as [wave][row][column]
constexpr int kLdsBytes = (kFoldWords + kWaves * kP4DecodeCols) * 4;      // ... and behind them their column sums
static_assert(kLdsBytes >= 16 * (kP4DecodeMaxSlice + kPad), "the A slice and the fold share the LDS");
static_assert(kThreads == 2 * kP4DecodeCols && kWaves == 4, "thread t finishes column t & 127 of the rows t >> 7, + 2, ...");

struct P4DecodeArgs : QdqArgs {       // A is unused (X below is quantized in the kernel); B / ldb: W and its leading dimension in bytes
    const float* X;
    int64_t ldx;
    int32_t x_vec;                    // rows of X are 16-byte aligned
    const float* q_scale;             // what the quantizer divides by: x_scale, or `safe` of a dynamic input
    const uint8_t* w_zp;              // one byte per tensor / column, NULL: 0
    int32_t w_per_column;
    uint32_t nibble_flip;             // 0x88888888 for a signed W
    uint32_t slice;                   // k of a workgroup, a multiple of 64
    int32_t w_near;                   // 48 rows of W lie inside 2^31 bytes: a lane's offset from its wave's row fits 32 bits
};

// r[i]: bytes of columns j = 0 ... 3 at k + i  ->  c[j]: bytes of k ... k + 3 of column j (qdq_function_packed4.hip)
__device__ __forceinline__ void transpose4x4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&c)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
    const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// four unsigned nibbles as bytes minus four zero points as bytes, byte by byte: each byte the two's complement of w - z
__device__ __forceinline__ uint32_t sub_bytes(uint32_t w4, uint32_t z4) { return ((w4 | 0x80808080u) - z4) ^ 0x80808080u; }

template <bool SUMS>
__global__ __launch_bounds__(kThreads) void qpd_product_kernel(const P4DecodeArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
    __shared__ float mm_red[2 * kWaves];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(tid >> 6));
    const uint32_t n0 = blockIdx.x * kP4DecodeCols, pn = n0 + 8u * c;                       // below 2^31 + a block
    const uint32_t k_begin = blockIdx.y * p.slice, k_end = min(p.K, k_begin + p.slice);    // below K + a slice
    const uint32_t quarter = p.slice / 4u;                                                 // a multiple of 16
    const uint32_t kb = min(k_end, k_begin + wave * quarter), ke = min(k_end, kb + quarter);
    const uint32_t stride = p.slice + kPad;

    // ---- A: the workgroup's slice of X, quantized, flipped, as [16][stride] bytes; 16-byte chunks, a row's chunks on neighbouring threads
    {
        const uint32_t chunks = (k_end - k_begin + 15u) / 16u;
        const QuantParams qp{p.q_scale[0], static_cast<float>(read_zp(p.a_zp, p.a_signed, 0)), p.a_signed ? -128.0f : 0.0f,
                             p.a_signed ? 127.0f : 255.0f};
        for (uint32_t id = tid; id < 16u * chunks; id += kThreads) {
            const uint32_t row = id / chunks, ch = id - row * chunks;
            u32x4 v{0u, 0u, 0u, 0u};
            if (row < p.M)
                v = quant_k16(p.X + static_cast<int64_t>(row) * p.ldx, k_begin + 16u * ch, p.K, p.x_vec != 0, qp, p.a_flip) ^
                    u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
            *reinterpret_cast<u32x4*>(lds + row * stride + 16u * ch) = v;
        }
    }

    // ---- B: this lane's dword of a row -- the columns pn ... pn + 7 -- and their zero points
    const bool alive = pn < p.N;
    const bool b_dword = p.b_vec != 0 && pn + 8u <= p.N;
    const bool block_dwords = p.b_vec != 0 && p.w_near != 0 && n0 + kP4DecodeCols <= p.N;      // the same for every lane of the workgroup
    const int b_last = static_cast<int>(min(3u, ((p.N - min(pn, p.N - 2u)) >> 1) - 1u));         // N is even: the last byte of the lane that exists
    const int o1 = min(1, b_last), o2 = min(2, b_last);
    uint32_t ze, zo;                     // the flipped zero points of the even / odd four of the eight columns
    if (p.w_zp != nullptr && alive) {
        uint32_t raw[2] = {0u, 0u};
        const uint8_t* z = p.w_zp + (p.w_per_column ? pn : 0u);      // walks the eight columns and stays on the last one that exists
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            raw[i >> 2] |= static_cast<uint32_t>(*z) << (8 * (i & 3));
            if (p.w_per_column && pn + i + 1 < p.N) ++z;
        }
        raw[0] = (raw[0] ^ p.nibble_flip) & 0x0F0F0F0Fu, raw[1] = (raw[1] ^ p.nibble_flip) & 0x0F0F0F0Fu;
        ze = __builtin_amdgcn_perm(raw[1], raw[0], 0x06040200u), zo = __builtin_amdgcn_perm(raw[1], raw[0], 0x07050301u);
    } else {
        ze = zo = p.nibble_flip & 0x0F0F0F0Fu;      // a missing zero point is the flip of 0
    }
    const uint32_t z_dword = (ze | (zo << 4)) ^ p.nibble_flip;      // the dword of a row that holds the zero points: B = 0

    // the wave's first row is a scalar address, the lane's place from there a 32-bit offset (block_dwords only)
    const uint8_t* const wave_row = p.B + static_cast<int64_t>(kb) * p.ldb + (n0 >> 1);
    const uint32_t lane_off = static_cast<uint32_t>(16 * g) * static_cast<uint32_t>(p.ldb) + 4u * c;

    auto load_span = [&](uint32_t (&r)[16], uint32_t s) {
        const uint32_t k0 = kb + kP4DecodeSpan * s;
        if (block_dwords && k0 + kP4DecodeSpan <= ke) {      // whole dwords of rows that all exist: nothing to guard
            const uint8_t* const row = wave_row + static_cast<int64_t>(kP4DecodeSpan * s) * p.ldb;
#pragma unroll
            for (int i = 0; i < 16; ++i) r[i] = *reinterpret_cast<const uint32_t*>(row + i * p.ldb + lane_off);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t kk = k0 + 16u * g + i;
                r[i] = z_dword;
                if (alive && kk < ke) {
                    const uint8_t* const src = p.B + static_cast<int64_t>(kk) * p.ldb + (pn >> 1);
                    if (b_dword) r[i] = *reinterpret_cast<const uint32_t*>(src);
                    else
                        r[i] = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[o1]) << 8) | (static_cast<uint32_t>(src[o2]) << 16) |
                               (static_cast<uint32_t>(src[b_last]) << 24);
                }
            }
        }
    };

    i32x4 acc[8], sums[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = sums[j] = i32x4{0, 0, 0, 0};
    const unsigned char* const a_frag = lds + c * stride + (kb - k_begin) + 16 * g;

    auto multiply_span = [&](const uint32_t (&r)[16], uint32_t s) {
        uint32_t col[8][4];      // col[j]: the 16 k of column pn + j
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t e[4], o[4], even[4], odd[4];      // even[j]: 4 k of column pn + 2 j;  odd[j]: of column pn + 2 j + 1
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t d = r[4 * q + i] ^ p.nibble_flip;
                e[i] = sub_bytes(d & 0x0F0F0F0Fu, ze), o[i] = sub_bytes((d >> 4) & 0x0F0F0F0Fu, zo);
            }
            transpose4x4(e[0], e[1], e[2], e[3], even);
            transpose4x4(o[0], o[1], o[2], o[3], odd);
#pragma unroll
            for (int j = 0; j < 4; ++j) col[2 * j][q] = even[j], col[2 * j + 1][q] = odd[j];
        }
        const i32x4 a = *reinterpret_cast<const i32x4*>(a_frag + kP4DecodeSpan * s);
        constexpr int kOnes = 0x01010101;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x4 b{static_cast<int>(col[j][0]), static_cast<int>(col[j][1]), static_cast<int>(col[j][2]), static_cast<int>(col[j][3])};
            acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[j], 0, 0, 0);
            if constexpr (SUMS) sums[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(i32x4{kOnes, kOnes, kOnes, kOnes}, b, sums[j], 0, 0, 0);
        }
    };

    const uint32_t spans = (ke - kb + kP4DecodeSpan - 1u) / kP4DecodeSpan;      // the same for every lane of the wave
    uint32_t next[16];
    if (spans) load_span(next, 0u);
    __syncthreads();      // the A slice is whole
    for (uint32_t s = 0; s < spans; ++s) {
        uint32_t now[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) now[i] = next[i];
        if (s + 1u < spans) load_span(next, s + 1u);
        multiply_span(now, s);
    }
    __syncthreads();      // behind every read of the A slice: LDS is free

    // ---- the fold.  C/D map of the 16x16 MFMAs: column index = lane & 15 -- column 8 c + j of the block --, row = 4 (lane >> 4) + r
    uint32_t* const fold = reinterpret_cast<uint32_t*>(lds);
    uint32_t* const fold_sums = fold + kFoldWords;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        i32x4* const dst = reinterpret_cast<i32x4*>(fold + (wave * 16u + 4u * g + r) * kP4DecodeCols + 8u * c);
        dst[0] = i32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]}, dst[1] = i32x4{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
    }
    if (SUMS && g == 0) {      // row 0 of the product with the ones
        i32x4* const dst = reinterpret_cast<i32x4*>(fold_sums + wave * kP4DecodeCols + 8u * c);
        dst[0] = i32x4{sums[0][0], sums[1][0], sums[2][0], sums[3][0]}, dst[1] = i32x4{sums[4][0], sums[5][0], sums[6][0], sums[7][0]};
    }
    __syncthreads();

    const uint32_t nl = tid & (kP4DecodeCols - 1), n = n0 + nl;
    MinMax mm;
    if (n < p.N) {
        uint32_t correction = 0u;      // zp_x' * sum_k B[k, n] over the slice
        if constexpr (SUMS) {
            uint32_t cs = 0u;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) cs += fold_sums[w * kP4DecodeCols + nl];
            correction = shifted_a_zp(p) * cs;
        }
        ColTerms ct{};
        float bias = 0.0f;
        if (!p.slab) ct = col_terms(p, n), bias = qdq_bias(p, n);      // colsum is NULL and B has no zero point: `add` is 0
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t m = (tid >> 7) + 2u * i;
            if (m < p.M) {
                uint32_t S = 0u;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) S += fold[(w * 16u + m) * kP4DecodeCols + nl];
                S -= correction;
                if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = S;
                else finish_qdq(p, m, n, S, ct, bias, mm);
            }
        }
    }
    if (!p.slab && p.out_mode == kQdqDynamic) block_minmax_store(mm, mm_red, p.pairs, blockIdx.x);
}

struct P4DecodeLayout : P4DecodePlan {      // and the workspace: include/oq_hip_qdq_function_packed4_decode.h, `workspace`: S, P, PX, PO
    uint32_t* slab;
    ParamBlock* params;
    float* x_pairs;
    float* out_pairs;
};

P4DecodeLayout make_layout(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode, Workspace& ws) {
    P4DecodeLayout pl{make_p4_decode_plan(M, K, N)};
    pl.slab = ws.take<uint32_t>(pl.slab_bytes);
    pl.params = x_mode == OQ_QDQ_DYNAMIC ? ws.take<ParamBlock>(sizeof(ParamBlock)) : nullptr;
    pl.x_pairs = x_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.x_blocks) * 8) : nullptr;
    pl.out_pairs = out_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.out_blocks) * 8) : nullptr;
    return pl;
}

bool request_ok(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    return shape_ok(M, K, N) && M <= kP4DecodeMaxRows && K <= kMaxK && N % 2 == 0 && (x_mode == OQ_QDQ_STATIC || x_mode == OQ_QDQ_DYNAMIC) &&
           mode_ok(out_mode);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_function_packed4_decode_extension_version(void) { return OQ_QDQ_FUNCTION_PACKED4_DECODE_EXTENSION_VERSION; }

size_t oq_qdq_function_packed4_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    if (!request_ok(M, K, N, x_mode, out_mode)) {
        set_error("oq_qdq_function_packed4_decode_workspace_bytes: M=%lld K=%lld N=%lld x_mode=%d out_mode=%d outside the bounds (M <= %d, K <= %lld, "
                  "an even N)", (long long)M, (long long)K, (long long)N, x_mode, out_mode, kP4DecodeMaxRows, (long long)kMaxK);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_layout(M, K, N, x_mode, out_mode, ws);
    return ws.total();
}

int32_t oq_qdq_function_packed4_decode(const void* X, int32_t atype, int64_t M, int64_t K, int64_t lda, int32_t x_mode, int32_t x_type,
                                       const float* x_scale, const void* x_zero_point, const void* W, int32_t wtype, int64_t N, int64_t ldw,
                                       int32_t granularity, int64_t group_size, const float* w_scale, const void* w_zero_point, const int32_t* B,
                                       const float* b_scale, const int32_t* b_zero_point, int32_t out_mode, int32_t out_type, const float* out_scale,
                                       const void* out_zero_point, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qdq_function_packed4_decode";
    // the checks of oq_qdq_function_packed4, in its order and with its status codes; the rows of this route behind the shape
    OQ_REQUIRE(X && W && Y, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (X, W and Y are required)", fn);
    OQ_REQUIRE(atype == OQ_NBITS_F32 || atype == OQ_NBITS_F16 || atype == OQ_NBITS_BF16, OQ_ERR_INVALID_ARGUMENT, "%s: unknown atype %d", fn, atype);
    OQ_REQUIRE(wtype == OQ_UINT8 || wtype == OQ_INT8 || wtype == OQ_UINT4 || wtype == OQ_INT4, OQ_ERR_INVALID_ARGUMENT, "%s: unknown wtype %d", fn, wtype);
    OQ_REQUIRE(granularity == OQ_TENSOR || granularity == OQ_CHANNEL || granularity == OQ_GROUP, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown granularity %d", fn, granularity);
    OQ_REQUIRE(x_mode == OQ_QDQ_STATIC || x_mode == OQ_QDQ_DYNAMIC, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown x_mode %d (OQ_QDQ_STATIC or OQ_QDQ_DYNAMIC: a function without an input Q -> DQ keeps oq_qdq_matmul_packed4)", fn, x_mode);
    OQ_REQUIRE(mode_ok(out_mode), OQ_ERR_INVALID_ARGUMENT, "%s: unknown out_mode %d", fn, out_mode);
    OQ_REQUIRE(x_mode != OQ_QDQ_STATIC || type_ok(x_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown x_type %d", fn, x_type);
    OQ_REQUIRE(out_mode != OQ_QDQ_STATIC || type_ok(out_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown out_type %d", fn, out_type);
    OQ_REQUIRE(w_scale && (x_mode != OQ_QDQ_STATIC || x_scale), OQ_ERR_INVALID_ARGUMENT,
               "%s: null pointer (w_scale is required, x_scale for a static input)", fn);
    OQ_REQUIRE(out_mode != OQ_QDQ_STATIC || out_scale, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (out_scale is required for a static output)", fn);
    OQ_REQUIRE(!B || b_scale, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (b_scale is required with a bias B)", fn);
    OQ_REQUIRE(extent_ok(M) && extent_ok(K) && extent_ok(N) && matrix_ok(M, K, lda) && matrix_ok(M, N, ldy), OQ_ERR_INVALID_ARGUMENT,
               "%s: M=%lld K=%lld N=%lld lda=%lld ldy=%lld outside the bounds", fn, (long long)M, (long long)K, (long long)N, (long long)lda,
               (long long)ldy);
    OQ_REQUIRE(shape_ok(M, K, N), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld: an operand beyond 2^40 elements", fn, (long long)M,
               (long long)K, (long long)N);
    OQ_REQUIRE(M <= kP4DecodeMaxRows, OQ_ERR_UNSUPPORTED, "%s: M = %lld rows (the decode route takes 1 ... %d; oq_qdq_function_packed4 is the entry point)",
               fn, (long long)M, kP4DecodeMaxRows);
    OQ_REQUIRE(atype == OQ_NBITS_F32, OQ_ERR_UNSUPPORTED, "%s: an fp16 / bf16 X has no kernel (atype %d; OQ_NBITS_F32 has one)", fn, atype);
    OQ_REQUIRE(granularity != OQ_GROUP, OQ_ERR_UNSUPPORTED, "%s: a grouped W (OQ_GROUP, group_size %lld) has no kernel; oq_qdq_matmul_packed4 takes it",
               fn, (long long)group_size);
    OQ_REQUIRE(wtype == OQ_UINT4 || wtype == OQ_INT4, OQ_ERR_UNSUPPORTED,
               "%s: an 8-bit W (wtype %d: one value per byte) keeps oq_qdq_function; OQ_UINT4 and OQ_INT4, two values per byte, have a kernel here", fn,
               wtype);
    OQ_REQUIRE(N % 2 == 0, OQ_ERR_UNSUPPORTED, "%s: N = %lld is odd (the rows of a flat-packed [K, N] start on alternating nibbles: no byte matrix)", fn,
               (long long)N);
    OQ_REQUIRE(matrix_ok(K, N / 2, ldw), OQ_ERR_INVALID_ARGUMENT, "%s: K=%lld N=%lld ldw=%lld outside the bounds (ldw counts bytes, >= N / 2)", fn,
               (long long)K, (long long)N, (long long)ldw);
    OQ_REQUIRE(K <= kMaxK, OQ_ERR_UNSUPPORTED, "%s: K = %lld: beyond %lld an int32 sum of products of an 8-bit and a 4-bit difference could wrap", fn,
               (long long)K, (long long)kMaxK);
    OQ_REQUIRE(aligned_to(X, 4) && aligned_to(Y, 4) && aligned_to(B, 4) && aligned_to(b_zero_point, 4) && aligned_to(x_scale, 4) &&
                   aligned_to(w_scale, 4) && aligned_to(b_scale, 4) && aligned_to(out_scale, 4),
               OQ_ERR_INVALID_ARGUMENT, "%s: X, Y, B, b_zero_point and the scales must be aligned to their element", fn);

    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const P4DecodeLayout pl = make_layout(M, K, N, x_mode, out_mode, ws);
    OQ_REQUIRE(ws.total() == 0 || ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    const bool dynamic_x = x_mode == OQ_QDQ_DYNAMIC;
    const float* const x = static_cast<const float*>(X);
    const int32_t x_vec = aligned_to(X, 16) && lda % 4 == 0;
    const void* const a_zp = dynamic_x ? static_cast<const void*>(&pl.params->zp) : x_zero_point;

    P4DecodeArgs p{};      // the epilogue's B: signed, no zero point -- W's zero points are subtracted in the registers
    fill_operands(p, nullptr, dynamic_x ? OQ_QL_U8 : x_type, M, K, 0, dynamic_x ? &pl.params->scale : x_scale, a_zp, W, OQ_QL_I8, OQ_QL_KN, N, ldw,
                  w_scale, nullptr, granularity == OQ_CHANNEL, nullptr, out_scale, out_zero_point, OQ_QL_OUT_F32, Y, ldy);
    p.slab = pl.slab;      // rowsum, colsum: NULL -- the product kernel corrects S itself
    p.bias = B, p.bias_scale = b_scale, p.bias_zp = b_zero_point;
    p.out_mode = out_mode, p.out_signed = out_mode == OQ_QDQ_STATIC && out_type == OQ_QL_I8, p.pairs = pl.out_pairs;
    p.X = x, p.ldx = lda, p.x_vec = x_vec, p.q_scale = dynamic_x ? &pl.params->safe : x_scale;
    p.w_zp = static_cast<const uint8_t*>(w_zero_point), p.w_per_column = granularity == OQ_CHANNEL;
    p.nibble_flip = wtype == OQ_INT4 ? 0x88888888u : 0u;
    p.slice = static_cast<uint32_t>(pl.slice), p.w_near = ldw < (int64_t{1} << 25);

    int32_t st;
    if (dynamic_x) {
        qq_minmax_rows_kernel<<<static_cast<unsigned>(pl.x_blocks), kThreads, 0, s>>>(x, p.M, p.K, lda, x_vec, pl.x_pairs);
        st = check_launch("qq_minmax_rows_kernel");
        if (st != OQ_OK) return st;
        qq_params_kernel<<<1, kThreads, 0, s>>>(pl.x_pairs, static_cast<uint32_t>(pl.x_blocks), pl.params);
        st = check_launch("qq_params_kernel");
        if (st != OQ_OK) return st;
    }
    const dim3 grid(static_cast<unsigned>(pl.col_blocks), static_cast<unsigned>(pl.splits));
    if (sum_needed(p.a_signed, a_zp)) qpd_product_kernel<true><<<grid, kThreads, 0, s>>>(p);
    else qpd_product_kernel<false><<<grid, kThreads, 0, s>>>(p);      // zp_x' is zero whatever the device holds
    st = check_launch("qpd_product_kernel");
    if (st != OQ_OK) return st;
    if (pl.splits > 1) {
        qq_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kThreads)), kThreads, 0, s>>>(p, static_cast<int>(pl.splits));
        st = check_launch("qq_reduce_kernel");
        if (st != OQ_OK) return st;
    }
    if (out_mode != OQ_QDQ_DYNAMIC) return OQ_OK;
    const int32_t y_vec = aligned_to(Y, 16) && ldy % 4 == 0 && N % 4 == 0;
    const int64_t work = y_vec ? M * (N / 4) : M * N;
    qq_finish_dynamic_kernel<<<static_cast<unsigned>(std::min<int64_t>(ceil_div(work, kThreads), 2048)), kThreads, 0, s>>>(
        Y, p.M, p.N, ldy, y_vec, pl.out_pairs, static_cast<uint32_t>(pl.out_blocks));
    return check_launch("qq_finish_dynamic_kernel");
}

}  // extern "C"
