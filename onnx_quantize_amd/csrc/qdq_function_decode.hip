// The decode route of a `quant`-domain QDQ function with quantized activations on an 8-bit weight (include/oq_hip_qdq_function_decode.h,
// DESIGN.md 4.36): the call of qdq_function.hip for 1 ... 16 rows of X.  W -- [K, N] bytes, as the file stores them -- is read once,
// from global memory straight into the registers that feed v_mfma_i32_16x16x64_i8.
//
//       q_x[m, k] = the static quantizer, or DynamicQuantizeLinear's with the parameters of X          quant_k16, qlinear_epilogue.hpp
//       a' = q_x ^ 0x80 [uint8], b' = W ^ 0x80 [uint8]: signed bytes;  za' = zp_x - 128 [uint8], zb'[n] = zp_w[n] - 128 [uint8]
//       S[m, n]   = sum a' b' - zb'[n] rowsum(a')[m] - za' colsum(b')[n] + K_s za' zb'[n]               exact, uint32 arithmetic
//       Y         = finish_qdq on S, with B signed and without a zero point: the epilogue text of qdq_function.hip
//
//   split     grid (ceil(N / 128), splits): a workgroup takes 128 columns and one slice of K (the plan: qdq_function_decode_plan.hpp),
//             its four waves a quarter of the slice each, in spans of 64 k.
//   A         the workgroup quantizes its slice of X into LDS as [16][slice + kPad] int8, flipped on the way in; rows >= M are zeros.
//             kPad = 80: a row is an odd number of 16-byte bank quads, so the 16 rows a 16-lane group reads lie in 16 different
//             quads, and a wave whose quarter is no whole span may read up to 48 bytes past its quarter inside the row.  One 16-byte
//             LDS read per span is the lane's A fragment: lane & 15 the row, lane >> 4 the 16-k chunk.
//   B         lane l: group g = l >> 4, column slot c = l & 15.  Per span the lane loads 8 bytes -- the columns 8 c ... 8 c + 7 of the
//             block -- of the 16 rows 64 s + 16 g ... + 15: a 16-lane group lies on one whole 128-byte line of a row.  The bytes are
//             flipped and four rows at a time go through the v_perm_b32 4 x 4 byte transpose (the text of
//             qdq_function_packed4_decode.hip), the low and the high dword each: eight transposes give, per column, the 16
//             consecutive k of the lane's rows as four dwords -- the lane's share of the matrix instruction's B operand (column index
//             lane & 15, k chunk lane >> 4).  So MFMA number j of a span multiplies the 16 columns {8 c + j}; its result column
//             lane & 15 is column 8 (lane & 15) + j of the block: an index in the epilogue.
//   pipeline  the 16 loads of span s + 1 are issued before the arithmetic of span s, into the other of two register sets: nothing
//             is consumed where it is loaded and nothing is copied.
//   sums      COLS: one more MFMA per B operand against an A of ones: every row of its result is colsum(b') over the wave's k.
//             ROWS: one MFMA per span of the A fragment against a B of ones: every column of its result is rowsum(a').  Both land
//             in the C / D layout of the products, so a lane corrects the 32 sums it holds from its own registers.
//   guards    a row k at or beyond the wave's end takes no load: its register holds the zero points of its columns as stored, so
//             that b' = zb' there.  What a' meets it (the next quarter, or bytes behind the slice that nobody wrote) then cancels
//             exactly: it enters sum a' b' and zb' rowsum(a') alike, both taken from the same fragment; K_s counts the wave's spans
//             whole, 64 each.  Without ROWS zb' is zero and so is b' there.  A lane whose columns lie at or beyond N loads nothing.
//             A last 8 bytes partly beyond N, and every row where W's rows are not 8-byte aligned, is read byte by byte; a column
//             at or beyond N (never stored) holds its zero point.
//   fold      the waves leave their corrected 16 x 128 sums in LDS, which the A slice no longer needs; thread t then adds the four
//             of column t & 127 for the rows t >> 7, + 2, ... and writes the slab (splits > 1: qq_reduce_kernel of
//             qdq_function_parts.hpp adds the slabs and finishes) or finishes through finish_qdq.
// Built with the library's flags alone, like qdq_function.hip: the same epilogue, the same bytes.
#include "qdq_function_parts.hpp"
#include "qdq_function_decode_plan.hpp"

#include "../../include/oq_hip_qdq_function_decode.h"

namespace oq {
namespace {

constexpr int64_t kMaxK = 33025;      // 255 * 255 * K <= 2^31 - 1: no int32 sum can wrap
constexpr int kPad = 80;              // bytes behind a row of the A slice in LDS
constexpr int kFoldWords = kWaves * 16 * kQfDecodeCols;      // the waves' sums as [wave][row][column]
constexpr int kSliceBytes = 16 * (kQfDecodeMaxSlice + kPad);
constexpr int kLdsBytes = kFoldWords * 4 > kSliceBytes ? kFoldWords * 4 : kSliceBytes;      // the A slice and the fold share the LDS
static_assert(kThreads == 2 * kQfDecodeCols && kWaves == 4, "thread t finishes column t & 127 of the rows t >> 7, + 2, ...");

struct QfDecodeArgs : QdqArgs {       // A is unused (X below is quantized in the kernel); B / ldb: W and its leading dimension
    const float* X;
    int64_t ldx;
    int32_t x_vec;                    // rows of X are 16-byte aligned
    const float* q_scale;             // what the quantizer divides by: x_scale, or `safe` of a dynamic input
    const uint8_t* w_zp;              // one byte per tensor / column, NULL: 0
    int32_t w_per_column;
    uint32_t w_flip;                  // 0x80808080 for an unsigned W
    uint32_t slice;                   // k of a workgroup, a multiple of 64
    int32_t w_vec;                    // W and its rows are 8-byte aligned
    int32_t w_near;                   // 64 rows of W lie inside 2^31 bytes: a lane's offset from its wave's row fits 32 bits
};

// r[i]: bytes of columns j = 0 ... 3 at k + i  ->  c[j]: bytes of k ... k + 3 of column j (qdq_function_packed4_decode.hip)
__device__ __forceinline__ void transpose4x4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&c)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
    const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// ROWS: zb' can be other than zero (the row sums of a' are needed); COLS: za' can be (the column sums of b' are)
template <bool ROWS, bool COLS>
__global__ __launch_bounds__(kThreads, 2) void qfd_product_kernel(const QfDecodeArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
    __shared__ float mm_red[2 * kWaves];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(tid >> 6));
    const uint32_t n0 = blockIdx.x * kQfDecodeCols, pn = n0 + 8u * c;                       // below 2^31 + a block
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

    // ---- B: this lane's 8 bytes of a row -- the columns pn ... pn + 7 -- and their zero points as stored
    const bool alive = pn < p.N;
    const bool b_qword = p.w_vec != 0 && pn + 8u <= p.N;
    const bool block_qwords = p.w_vec != 0 && p.w_near != 0 && n0 + kQfDecodeCols <= p.N;      // the same for every lane of the workgroup
    u32x2 z_raw{0u, 0u};
    if (ROWS && p.w_zp != nullptr) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (pn + i < p.N) z_raw[i >> 2] |= static_cast<uint32_t>(p.w_zp[p.w_per_column ? pn + i : 0u]) << (8 * (i & 3));
    }

    // the wave's first row is a scalar address, the lane's place from there a 32-bit offset (block_qwords only)
    const uint8_t* const wave_row = p.B + static_cast<int64_t>(kb) * p.ldb + n0;
    const uint32_t lane_off = static_cast<uint32_t>(16 * g) * static_cast<uint32_t>(p.ldb) + 8u * c;

    auto load_span = [&](u32x2 (&r)[16], uint32_t s) {
        const uint32_t k0 = kb + kQfDecodeSpan * s;
        if (block_qwords && k0 + kQfDecodeSpan <= ke) {      // whole 8 bytes of rows that all exist: nothing to guard
            const uint8_t* const row = wave_row + static_cast<int64_t>(kQfDecodeSpan * s) * p.ldb;
#pragma unroll
            for (int i = 0; i < 16; ++i) r[i] = *reinterpret_cast<const u32x2*>(row + i * p.ldb + lane_off);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t kk = k0 + 16u * g + i;
                r[i] = z_raw;
                if (alive && kk < ke) {
                    const uint8_t* const src = p.B + static_cast<int64_t>(kk) * p.ldb + pn;
                    if (b_qword) r[i] = *reinterpret_cast<const u32x2*>(src);
                    else {
#pragma unroll
                        for (int b = 0; b < 8; ++b)
                            if (pn + b < p.N)
                                r[i][b >> 2] = (r[i][b >> 2] & ~(0xFFu << (8 * (b & 3)))) | (static_cast<uint32_t>(src[b]) << (8 * (b & 3)));
                    }
                }
            }
        }
    };

    i32x4 acc[8], sums[8], rs{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = sums[j] = i32x4{0, 0, 0, 0};
    const unsigned char* const a_frag = lds + c * stride + (kb - k_begin) + 16 * g;

    auto multiply_span = [&](const u32x2 (&r)[16], uint32_t s) {
        uint32_t col[8][4];      // col[j]: the 16 k of column pn + j
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t lo[4], hi[4];      // lo[j]: 4 k of column pn + j;  hi[j]: of column pn + 4 + j
            transpose4x4(r[4 * q][0] ^ p.w_flip, r[4 * q + 1][0] ^ p.w_flip, r[4 * q + 2][0] ^ p.w_flip, r[4 * q + 3][0] ^ p.w_flip, lo);
            transpose4x4(r[4 * q][1] ^ p.w_flip, r[4 * q + 1][1] ^ p.w_flip, r[4 * q + 2][1] ^ p.w_flip, r[4 * q + 3][1] ^ p.w_flip, hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) col[j][q] = lo[j], col[4 + j][q] = hi[j];
        }
        const i32x4 a = *reinterpret_cast<const i32x4*>(a_frag + kQfDecodeSpan * s);
        constexpr int kOnes = 0x01010101;
        const i32x4 ones{kOnes, kOnes, kOnes, kOnes};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x4 b{static_cast<int>(col[j][0]), static_cast<int>(col[j][1]), static_cast<int>(col[j][2]), static_cast<int>(col[j][3])};
            acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[j], 0, 0, 0);
            if constexpr (COLS) sums[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, sums[j], 0, 0, 0);
        }
        if constexpr (ROWS) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, rs, 0, 0, 0);
    };

    const uint32_t spans = (ke - kb + kQfDecodeSpan - 1u) / kQfDecodeSpan;      // the same for every lane of the wave
    u32x2 even[16], odd[16];      // the spans 0, 2, ... and 1, 3, ...
    if (spans) load_span(even, 0u);
    __syncthreads();      // the A slice is whole
    for (uint32_t s = 0; s < spans; s += 2u) {
        if (s + 1u < spans) load_span(odd, s + 1u);
        multiply_span(even, s);
        if (s + 1u < spans) {
            if (s + 2u < spans) load_span(even, s + 2u);
            multiply_span(odd, s + 1u);
        }
    }
    __syncthreads();      // behind every read of the A slice: LDS is free

    // ---- the correction, in the C / D map of the 16x16 MFMAs: column index = lane & 15 -- column 8 c + j of the block --, row =
    // 4 (lane >> 4) + r: rs[r] is rowsum(a') of the row of acc[j][r], sums[j][r] colsum(b') of its column
    if constexpr (ROWS || COLS) {
        const uint32_t za = COLS ? shifted_a_zp(p) : 0u;
        const u32x2 z_flipped = z_raw ^ u32x2{p.w_flip, p.w_flip};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t zb = static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(z_flipped[j >> 2] >> (8 * (j & 3)))));
            const uint32_t k_term = kQfDecodeSpan * spans * za * zb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint32_t v = static_cast<uint32_t>(acc[j][r]) + k_term;
                if constexpr (ROWS) v -= zb * static_cast<uint32_t>(rs[r]);
                if constexpr (COLS) v -= za * static_cast<uint32_t>(sums[j][r]);
                acc[j][r] = static_cast<int32_t>(v);
            }
        }
    }

    // ---- the fold
    uint32_t* const fold = reinterpret_cast<uint32_t*>(lds);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        i32x4* const dst = reinterpret_cast<i32x4*>(fold + (wave * 16u + 4u * g + r) * kQfDecodeCols + 8u * c);
        dst[0] = i32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]}, dst[1] = i32x4{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
    }
    __syncthreads();

    const uint32_t nl = tid & (kQfDecodeCols - 1), n = n0 + nl;
    MinMax mm;
    if (n < p.N) {
        ColTerms ct{};
        float bias = 0.0f;
        if (!p.slab) ct = col_terms(p, n), bias = qdq_bias(p, n);      // colsum is NULL and B has no zero point: `add` is 0
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t m = (tid >> 7) + 2u * i;
            if (m < p.M) {
                uint32_t S = 0u;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) S += fold[(w * 16u + m) * kQfDecodeCols + nl];
                if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = S;
                else finish_qdq(p, m, n, S, ct, bias, mm);
            }
        }
    }
    if (!p.slab && p.out_mode == kQdqDynamic) block_minmax_store(mm, mm_red, p.pairs, blockIdx.x);
}

struct QfDecodeLayout : QfDecodePlan {      // and the workspace: include/oq_hip_qdq_function_decode.h, `workspace`: S, P, PX, PO
    uint32_t* slab;
    ParamBlock* params;
    float* x_pairs;
    float* out_pairs;
};

QfDecodeLayout make_layout(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode, Workspace& ws) {
    QfDecodeLayout pl{make_qf_decode_plan(M, K, N)};
    pl.slab = ws.take<uint32_t>(pl.slab_bytes);
    pl.params = x_mode == OQ_QDQ_DYNAMIC ? ws.take<ParamBlock>(sizeof(ParamBlock)) : nullptr;
    pl.x_pairs = x_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.x_blocks) * 8) : nullptr;
    pl.out_pairs = out_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.out_blocks) * 8) : nullptr;
    return pl;
}

bool request_ok(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    return shape_ok(M, K, N) && M <= kQfDecodeMaxRows && K <= kMaxK && (x_mode == OQ_QDQ_STATIC || x_mode == OQ_QDQ_DYNAMIC) && mode_ok(out_mode);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_function_decode_extension_version(void) { return OQ_QDQ_FUNCTION_DECODE_EXTENSION_VERSION; }

size_t oq_qdq_function_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    if (!request_ok(M, K, N, x_mode, out_mode)) {
        set_error("oq_qdq_function_decode_workspace_bytes: M=%lld K=%lld N=%lld x_mode=%d out_mode=%d outside the bounds (M <= %d, K <= %lld)",
                  (long long)M, (long long)K, (long long)N, x_mode, out_mode, kQfDecodeMaxRows, (long long)kMaxK);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_layout(M, K, N, x_mode, out_mode, ws);
    return ws.total();
}

int32_t oq_qdq_function_decode(const void* X, int32_t atype, int64_t M, int64_t K, int64_t lda, int32_t x_mode, int32_t x_type, const float* x_scale,
                               const void* x_zero_point, const void* W, int32_t wtype, int64_t N, int64_t ldw, int32_t granularity,
                               int64_t group_size, const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale,
                               const int32_t* b_zero_point, int32_t out_mode, int32_t out_type, const float* out_scale, const void* out_zero_point,
                               float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qdq_function_decode";
    // the checks of oq_qdq_function, in its order and with its status codes; the rows of this route behind the shape
    OQ_REQUIRE(X && W && Y, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (X, W and Y are required)", fn);
    OQ_REQUIRE(atype == OQ_NBITS_F32 || atype == OQ_NBITS_F16 || atype == OQ_NBITS_BF16, OQ_ERR_INVALID_ARGUMENT, "%s: unknown atype %d", fn, atype);
    OQ_REQUIRE(wtype == OQ_UINT8 || wtype == OQ_INT8 || wtype == OQ_UINT4 || wtype == OQ_INT4, OQ_ERR_INVALID_ARGUMENT, "%s: unknown wtype %d", fn, wtype);
    OQ_REQUIRE(granularity == OQ_TENSOR || granularity == OQ_CHANNEL || granularity == OQ_GROUP, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown granularity %d", fn, granularity);
    OQ_REQUIRE(x_mode == OQ_QDQ_STATIC || x_mode == OQ_QDQ_DYNAMIC, OQ_ERR_INVALID_ARGUMENT,
               "%s: unknown x_mode %d (OQ_QDQ_STATIC or OQ_QDQ_DYNAMIC: a function without an input Q -> DQ keeps oq_qdq_matmul)", fn, x_mode);
    OQ_REQUIRE(mode_ok(out_mode), OQ_ERR_INVALID_ARGUMENT, "%s: unknown out_mode %d", fn, out_mode);
    OQ_REQUIRE(x_mode != OQ_QDQ_STATIC || type_ok(x_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown x_type %d", fn, x_type);
    OQ_REQUIRE(out_mode != OQ_QDQ_STATIC || type_ok(out_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown out_type %d", fn, out_type);
    OQ_REQUIRE(w_scale && (x_mode != OQ_QDQ_STATIC || x_scale), OQ_ERR_INVALID_ARGUMENT,
               "%s: null pointer (w_scale is required, x_scale for a static input)", fn);
    OQ_REQUIRE(out_mode != OQ_QDQ_STATIC || out_scale, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (out_scale is required for a static output)", fn);
    OQ_REQUIRE(!B || b_scale, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (b_scale is required with a bias B)", fn);
    OQ_REQUIRE(extent_ok(M) && extent_ok(K) && extent_ok(N) && matrix_ok(M, K, lda) && matrix_ok(K, N, ldw) && matrix_ok(M, N, ldy),
               OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld lda=%lld ldw=%lld ldy=%lld outside the bounds", fn, (long long)M, (long long)K,
               (long long)N, (long long)lda, (long long)ldw, (long long)ldy);
    OQ_REQUIRE(shape_ok(M, K, N), OQ_ERR_INVALID_ARGUMENT, "%s: M=%lld K=%lld N=%lld: an operand beyond 2^40 elements", fn, (long long)M,
               (long long)K, (long long)N);
    OQ_REQUIRE(M <= kQfDecodeMaxRows, OQ_ERR_UNSUPPORTED, "%s: M = %lld rows (the decode route takes 1 ... %d; oq_qdq_function is the entry point)", fn,
               (long long)M, kQfDecodeMaxRows);
    OQ_REQUIRE(atype == OQ_NBITS_F32, OQ_ERR_UNSUPPORTED, "%s: an fp16 / bf16 X has no kernel (atype %d; OQ_NBITS_F32 has one)", fn, atype);
    OQ_REQUIRE(granularity != OQ_GROUP, OQ_ERR_UNSUPPORTED, "%s: a grouped W (OQ_GROUP, group_size %lld) has no kernel; oq_qdq_matmul takes it", fn,
               (long long)group_size);
    OQ_REQUIRE(wtype == OQ_UINT8 || wtype == OQ_INT8, OQ_ERR_UNSUPPORTED,
               "%s: a 4-bit W (wtype %d) has no kernel here; oq_qdq_function_packed4_decode takes its packed nibbles", fn, wtype);
    OQ_REQUIRE(K <= kMaxK, OQ_ERR_UNSUPPORTED, "%s: K = %lld: beyond %lld an int32 sum of 8-bit products could wrap", fn, (long long)K,
               (long long)kMaxK);
    OQ_REQUIRE(aligned_to(X, 4) && aligned_to(Y, 4) && aligned_to(B, 4) && aligned_to(b_zero_point, 4) && aligned_to(x_scale, 4) &&
                   aligned_to(w_scale, 4) && aligned_to(b_scale, 4) && aligned_to(out_scale, 4),
               OQ_ERR_INVALID_ARGUMENT, "%s: X, Y, B, b_zero_point and the scales must be aligned to their element", fn);

    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const QfDecodeLayout pl = make_layout(M, K, N, x_mode, out_mode, ws);
    OQ_REQUIRE(ws.total() == 0 || ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    const bool dynamic_x = x_mode == OQ_QDQ_DYNAMIC;
    const float* const x = static_cast<const float*>(X);
    const int32_t x_vec = aligned_to(X, 16) && lda % 4 == 0;
    const void* const a_zp = dynamic_x ? static_cast<const void*>(&pl.params->zp) : x_zero_point;

    QfDecodeArgs p{};      // the epilogue's B: signed, no zero point -- the product kernel corrects S for W's zero points itself
    fill_operands(p, nullptr, dynamic_x ? OQ_QL_U8 : x_type, M, K, 0, dynamic_x ? &pl.params->scale : x_scale, a_zp, W, OQ_QL_I8, OQ_QL_KN, N, ldw,
                  w_scale, nullptr, granularity == OQ_CHANNEL, nullptr, out_scale, out_zero_point, OQ_QL_OUT_F32, Y, ldy);
    p.slab = pl.slab;      // rowsum, colsum: NULL
    p.bias = B, p.bias_scale = b_scale, p.bias_zp = b_zero_point;
    p.out_mode = out_mode, p.out_signed = out_mode == OQ_QDQ_STATIC && out_type == OQ_QL_I8, p.pairs = pl.out_pairs;
    p.X = x, p.ldx = lda, p.x_vec = x_vec, p.q_scale = dynamic_x ? &pl.params->safe : x_scale;
    p.w_zp = static_cast<const uint8_t*>(w_zero_point), p.w_per_column = granularity == OQ_CHANNEL;
    p.w_flip = wtype == OQ_INT8 ? 0u : 0x80808080u;
    p.slice = static_cast<uint32_t>(pl.slice), p.w_vec = aligned_to(W, 8) && ldw % 8 == 0, p.w_near = ldw < (int64_t{1} << 25);

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
    const bool rows = sum_needed(wtype == OQ_INT8, w_zero_point), cols = sum_needed(p.a_signed, a_zp);      // zb' / za' can be other than zero
    if (rows && cols) qfd_product_kernel<true, true><<<grid, kThreads, 0, s>>>(p);
    else if (rows) qfd_product_kernel<true, false><<<grid, kThreads, 0, s>>>(p);
    else if (cols) qfd_product_kernel<false, true><<<grid, kThreads, 0, s>>>(p);
    else qfd_product_kernel<false, false><<<grid, kThreads, 0, s>>>(p);
    st = check_launch("qfd_product_kernel");
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
