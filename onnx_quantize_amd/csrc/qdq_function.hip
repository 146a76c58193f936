// One call of a `quant`-domain QDQ function with quantized activations (include/oq_hip_qdq_function.h): fp32 X in,
// fp32 Y out, the product of the 8-bit q_x and the stored 8-bit W on the int8 matrix cores.
//
//       q_x[m, k] = the static quantizer (quant_k16), or DynamicQuantizeLinear's with the parameters of X
//       S[m, n]   = sum_k (q_x[m, k] - zp_x) * (W[k, n] - zp_w[n])                            exact, int32
//       v         = fp32(S) * fl(x_scale * w_scale[n])  (+ the dequantized bias)              finish_qdq (qlinear_epilogue.hpp)
//       Y         = v | the static Q -> DQ of v | the dynamic Q -> DQ of v
//
// The product is the tile GEMM body of qlinear_tile.hpp in the KN layout with the policy kEpQdqFunction; the prologue that quantizes X
// is the text of qlinear_function.hip's (a copy -- why: qlinear_tile.hpp), with its parameter pointers aimed at the workspace for a
// dynamic input.  New here: the min / max pass over X, the one-workgroup kernel that turns its pairs into parameters, and the launch
// that finishes a dynamic output.  The launches of each variant: the header.
#include "qlinear_tile.hpp"

#include "../../include/oq_hip_qdq_function.h"

namespace oq {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kMaxK = 33025;            // 255 * 255 * K <= 2^31 - 1: no int32 sum can wrap
constexpr int64_t kMaxPairBlocks = 2048;    // workgroups of the pass over X
constexpr int kWaves = kThreads / kWave;
static_assert(kQdqNone == OQ_QDQ_NONE && kQdqStatic == OQ_QDQ_STATIC && kQdqDynamic == OQ_QDQ_DYNAMIC, "the epilogue's modes are oq_qdq_mode's");

struct QdqArgs : QlArgs {
    const int32_t* bias;         // NULL: MatMul
    const float* bias_scale;
    const int32_t* bias_zp;      // NULL: 0
    int32_t out_mode, out_signed;
    float* pairs;                // a dynamic output: one (min, max) per workgroup that finishes v
};

// the parameter block of a dynamic input in the workspace: three dwords
struct ParamBlock {
    float safe, scale;
    uint32_t zp;                 // its low byte is the uint8 zero point (read_zp)
};

// ---- dynamic input
// pairs[2 b], pairs[2 b + 1] = (min, max) of the rows workgroup b takes: one wave per row, rows in turn.  Nothing at or beyond column
// K is read.  `vec`: rows are 16-byte aligned.
__global__ __launch_bounds__(kThreads) void qq_minmax_rows_kernel(const float* X, uint32_t M, uint32_t K, int64_t ldx, int32_t vec, float* pairs) {
    __shared__ float red[2 * kWaves];
    const uint32_t lane = threadIdx.x & 63;
    MinMax mm;
    for (uint32_t row = blockIdx.x * kWaves + (threadIdx.x >> 6); row < M; row += gridDim.x * kWaves) {      // the grid: at most 2048 blocks
        const float* x = X + static_cast<int64_t>(row) * ldx;
        uint32_t done = 0u;
        if (vec) {
            for (uint32_t k = 4u * lane; k + 4u <= K; k += 4u * kWave) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + k);
                mm.lo = nmin(nmin(mm.lo, v[0]), nmin(v[1], nmin(v[2], v[3])));
                mm.hi = nmax(nmax(mm.hi, v[0]), nmax(v[1], nmax(v[2], v[3])));
            }
            done = K & ~3u;
        }
        for (uint32_t k = done + lane; k < K; k += kWave) mm.lo = nmin(mm.lo, x[k]), mm.hi = nmax(mm.hi, x[k]);
    }
    block_minmax_store(mm, red, pairs, blockIdx.x);
}

// the fold of `count` pairs by one workgroup: every thread gets the result
__device__ __forceinline__ MinMax fold_pairs(const float* pairs, uint32_t count, float* red) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    MinMax mm;
    for (uint32_t i = threadIdx.x; i < count; i += kThreads) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(pairs + 2 * static_cast<int64_t>(i));
        mm.lo = nmin(mm.lo, v[0]), mm.hi = nmax(mm.hi, v[1]);
    }
    return block_minmax(mm, red);
}

// one workgroup: the pairs of the pass over X -> safe, scale, zp
__global__ __launch_bounds__(kThreads) void qq_params_kernel(const float* pairs, uint32_t count, ParamBlock* out) {
    __shared__ float red[2 * kWaves];
    const DynParams d = dyn_params(fold_pairs(pairs, count, red));
    if (threadIdx.x == 0) {
        typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
        *reinterpret_cast<u32x3*>(out) = u32x3{__float_as_uint(d.safe), __float_as_uint(d.scale), static_cast<uint32_t>(static_cast<int32_t>(d.zp))};
    }
}

// ---- the prologue: qf_quantize_rows_kernel of qlinear_function.hip
__global__ __launch_bounds__(kThreads) void qq_quantize_rows_kernel(const QlArgs p, const float* X, int64_t ldx, int32_t x_vec, uint8_t* Q,
                                                                    int32_t* sums) {
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);      // the grid is ceil(M / 4) blocks: below 2^31
    if (row >= p.M) return;
    const float* x = X + static_cast<int64_t>(row) * ldx;
    uint8_t* q = Q + static_cast<int64_t>(row) * p.lda;                             // lda: of the image, a multiple of 16
    const QuantParams qp = quant_of(p);
    uint32_t s = 0u;
    for (uint32_t k = 16u * lane; k < p.K; k += 16u * kWave) {                      // k + 16 <= r16(K) = lda
        const u32x4 v = quant_k16(x, k, p.K, x_vec != 0, qp, p.a_flip);
        *reinterpret_cast<u32x4*>(q + k) = v;
#pragma unroll
        for (int j = 0; j < 4; ++j)                                                 // past K: the flip's byte, a zero after the flip
            s = static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(v[j] ^ p.a_flip), 0x01010101, static_cast<int>(s), false));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s), off, kWave));
    if (sums && lane == 0) sums[row] = static_cast<int32_t>(s);
}

__global__ __launch_bounds__(kThreads) void qq_sum_cols_kernel(const uint8_t* X, int64_t K, int64_t N, int64_t ld, uint32_t ubias, int32_t vec,
                                                               int32_t* sums, int64_t stride) {
    __shared__ uint32_t part[16][64];
    ql_sum_cols_body(X, K, N, ld, ubias, vec, sums, stride, part);
}

// ---- the product
template <int MT>
__global__ __launch_bounds__(kThreads, 2) void qq_gemm_kernel(const QdqArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[ql_gemm_lds_bytes(MT)];
    ql_gemm_body<MT, OQ_QL_KN, kEpQdqFunction>(p, lds);
}

__global__ __launch_bounds__(kThreads) void qq_reduce_kernel(const QdqArgs p, const int splits) {
    __shared__ float red[2 * kWaves];
    ql_reduce_body<kEpQdqFunction>(p, splits, red);
}

// ---- dynamic output: the pairs of the workgroups that wrote v -> the parameters (every workgroup folds all pairs, in one order) ->
// Y = dq(q(v)) in place.  `vec`: Y and its rows are 16-byte aligned and N is a multiple of 4.
__global__ __launch_bounds__(kThreads) void qq_finish_dynamic_kernel(float* Y, uint32_t M, uint32_t N, int64_t ldy, int32_t vec, const float* pairs,
                                                                     uint32_t count) {
    __shared__ float red[2 * kWaves];
    const DynParams d = dyn_params(fold_pairs(pairs, count, red));
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (vec) {
        const uint32_t n4 = N / 4u;
        const int64_t total = static_cast<int64_t>(M) * n4;
        for (int64_t i = first; i < total; i += stride) {
            f32x4* const y = reinterpret_cast<f32x4*>(Y + (i / n4) * ldy + 4 * (i % n4));
            f32x4 v = *y;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = dyn_qdq(v[j], d);
            *y = v;
        }
    } else {
        const int64_t total = static_cast<int64_t>(M) * N;
        for (int64_t i = first; i < total; i += stride) {
            float* const y = Y + (i / N) * ldy + i % N;
            *y = dyn_qdq(*y, d);
        }
    }
}

// ---- host
bool mode_ok(int32_t m) { return m == OQ_QDQ_NONE || m == OQ_QDQ_STATIC || m == OQ_QDQ_DYNAMIC; }

struct QdqFunctionPlan : Plan {      // and the workspace: include/oq_hip_qdq_function.h, `workspace`: Q, R, C, S, then P, PX, PO
    uint8_t* image;                  // [M, ldq] the quantized X
    int64_t ldq;                     // K rounded up to 16
    ParamBlock* params;              // a dynamic input: safe, scale, zp
    float* x_pairs;                  // a dynamic input: [x_blocks] (min, max)
    int64_t x_blocks;
    float* out_pairs;                // a dynamic output: [out_blocks] (min, max)
    int64_t out_blocks;              // the workgroups that finish v
};

QdqFunctionPlan make_qdq_function_plan(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode, Workspace& ws) {
    const int64_t ldq = ceil_div(K, 16) * 16;
    uint8_t* const image = ws.take<uint8_t>(static_cast<size_t>(M) * static_cast<size_t>(ldq));
    QdqFunctionPlan pl{make_plan(M, K, N, ws)};
    pl.image = image, pl.ldq = ldq;
    pl.x_blocks = std::min<int64_t>(ceil_div(M, kWaves), kMaxPairBlocks);
    pl.out_blocks = pl.splits == 1 ? pl.tiles : ceil_div(M * N, kThreads);
    pl.params = x_mode == OQ_QDQ_DYNAMIC ? ws.take<ParamBlock>(sizeof(ParamBlock)) : nullptr;
    pl.x_pairs = x_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.x_blocks) * 8) : nullptr;
    pl.out_pairs = out_mode == OQ_QDQ_DYNAMIC ? ws.take<float>(static_cast<size_t>(pl.out_blocks) * 8) : nullptr;
    return pl;
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_function_extension_version(void) { return OQ_QDQ_FUNCTION_EXTENSION_VERSION; }

size_t oq_qdq_function_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    if (!shape_ok(M, K, N) || K > kMaxK || (x_mode != OQ_QDQ_STATIC && x_mode != OQ_QDQ_DYNAMIC) || !mode_ok(out_mode)) {
        set_error("oq_qdq_function_workspace_bytes: M=%lld K=%lld N=%lld x_mode=%d out_mode=%d outside the bounds", (long long)M, (long long)K,
                  (long long)N, x_mode, out_mode);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_qdq_function_plan(M, K, N, x_mode, out_mode, ws);
    return ws.total();
}

int32_t oq_qdq_function(const void* X, int32_t atype, int64_t M, int64_t K, int64_t lda, int32_t x_mode, int32_t x_type, const float* x_scale,
                        const void* x_zero_point, const void* W, int32_t wtype, int64_t N, int64_t ldw, int32_t granularity, int64_t group_size,
                        const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale, const int32_t* b_zero_point,
                        int32_t out_mode, int32_t out_type, const float* out_scale, const void* out_zero_point, float* Y, int64_t ldy, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qdq_function";
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
    OQ_REQUIRE(atype == OQ_NBITS_F32, OQ_ERR_UNSUPPORTED, "%s: an fp16 / bf16 X has no kernel (atype %d; OQ_NBITS_F32 has one)", fn, atype);
    OQ_REQUIRE(granularity != OQ_GROUP, OQ_ERR_UNSUPPORTED, "%s: a grouped W (OQ_GROUP, group_size %lld) has no kernel; oq_qdq_matmul takes it", fn,
               (long long)group_size);
    OQ_REQUIRE(wtype == OQ_UINT8 || wtype == OQ_INT8, OQ_ERR_UNSUPPORTED, "%s: a 4-bit W (wtype %d) has no kernel; oq_qdq_matmul takes it", fn, wtype);
    OQ_REQUIRE(K <= kMaxK, OQ_ERR_UNSUPPORTED, "%s: K = %lld: beyond %lld an int32 sum of 8-bit products could wrap", fn, (long long)K,
               (long long)kMaxK);
    OQ_REQUIRE(aligned_to(X, 4) && aligned_to(Y, 4) && aligned_to(B, 4) && aligned_to(b_zero_point, 4) && aligned_to(x_scale, 4) &&
                   aligned_to(w_scale, 4) && aligned_to(b_scale, 4) && aligned_to(out_scale, 4),
               OQ_ERR_INVALID_ARGUMENT, "%s: X, Y, B, b_zero_point and the scales must be aligned to their element", fn);

    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const QdqFunctionPlan pl = make_qdq_function_plan(M, K, N, x_mode, out_mode, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    const float* const x = static_cast<const float*>(X);
    const bool dynamic_x = x_mode == OQ_QDQ_DYNAMIC;
    const int32_t a_type = dynamic_x ? OQ_QL_U8 : x_type;
    // a dynamic input: the quantizer divides by `safe`, the product scales by `scale`; the zero point is the low byte of the block's dword
    const float* const quant_scale = dynamic_x ? &pl.params->safe : x_scale;
    const float* const prod_scale = dynamic_x ? &pl.params->scale : x_scale;
    const void* const a_zp = dynamic_x ? static_cast<const void*>(&pl.params->zp) : x_zero_point;
    const int32_t out_signed = out_mode == OQ_QDQ_STATIC && out_type == OQ_QL_I8;

    QdqArgs p{};      // the product's operand A is the image: bytes of a_type, rows 16-byte aligned; out F32: col_terms forms the scale
    fill_operands(p, pl.image, a_type, M, K, pl.ldq, prod_scale, a_zp, W, wtype == OQ_INT8 ? OQ_QL_I8 : OQ_QL_U8, OQ_QL_KN, N, ldw, w_scale,
                  w_zero_point, granularity == OQ_CHANNEL, nullptr, out_scale, out_zero_point, OQ_QL_OUT_F32, Y, ldy);
    p.tiles_m = static_cast<uint32_t>(pl.tiles_m), p.steps_per_split = static_cast<uint32_t>(pl.steps_per_split);
    int32_t* rowsum = sum_needed(p.b_signed, w_zero_point) ? pl.rowsum : nullptr;
    int32_t* colsum = sum_needed(p.a_signed, a_zp) ? pl.colsum : nullptr;
    p.rowsum = rowsum, p.colsum = colsum;
    p.colsum_slices = kColSlices, p.colsum_stride = pl.colsum_stride;
    p.slab = pl.slab;
    p.bias = B, p.bias_scale = b_scale, p.bias_zp = b_zero_point;
    p.out_mode = out_mode, p.out_signed = out_signed, p.pairs = pl.out_pairs;

    const int32_t x_vec = aligned_to(x, 16) && lda % 4 == 0;
    int32_t st;
    if (dynamic_x) {
        qq_minmax_rows_kernel<<<static_cast<unsigned>(pl.x_blocks), kThreads, 0, s>>>(x, p.M, p.K, lda, x_vec, pl.x_pairs);
        st = check_launch("qq_minmax_rows_kernel");
        if (st != OQ_OK) return st;
        qq_params_kernel<<<1, kThreads, 0, s>>>(pl.x_pairs, static_cast<uint32_t>(pl.x_blocks), pl.params);
        st = check_launch("qq_params_kernel");
        if (st != OQ_OK) return st;
    }
    QlArgs q = p;      // the prologue reads a_scale, a_zp, a_signed, a_flip, M, K and lda
    q.a_scale = quant_scale;
    qq_quantize_rows_kernel<<<static_cast<unsigned>(ceil_div(M, kWaves)), kThreads, 0, s>>>(q, x, lda, x_vec, pl.image, rowsum);
    st = check_launch("qq_quantize_rows_kernel");
    if (st != OQ_OK) return st;
    if (colsum) {      // over w ^ ubias read as an unsigned byte, minus 128: ubias flips a SIGNED operand (qlinear_gemm.hip)
        qq_sum_cols_kernel<<<dim3(static_cast<unsigned>(ceil_div(N, 64)), kColSlices), kThreads, 0, s>>>(p.B, K, N, ldw, p.b_flip ^ 0x80808080u,
                                                                                                          aligned_to(W, 4) && ldw % 4 == 0, colsum,
                                                                                                          p.colsum_stride);
        st = check_launch("qq_sum_cols_kernel");
        if (st != OQ_OK) return st;
    }
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { qq_gemm_kernel<decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
    st = check_launch("qq_gemm_kernel");
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
