// One call of a `quant`-domain function QLinearMatMul / QLinearGemm (include/oq_hip_qlinear_function.h): fp32 X in,
// fp32 Y out, the bytes of QuantizeLinear -> QLinearMatMul | QGemm -> DequantizeLinear run node by node.
//
//       q_a[m, k] = sat_a(rint(X[m, k] / a_scale) + fp32(a_zp))                        quant_k16 (qlinear_epilogue.hpp)
//       acc[m, n] = sum_k (q_a[m, k] - a_zp) * (B[k, n] - b_zp[n])  (+ C[n])           exact, int32
//       Y[m, n]   = (fp32(q_y) - fp32(y_zp)) * y_scale,  q_y the 8-bit epilogue        finish_acc<DQ>
//
// The product's kernels are the bodies of qlinear_tile.hpp and qlinear_decode_body.hpp with their flags on: the text of
// qlinear_gemm.hip's and qlinear_decode.hip's kernels (a copy -- why: those headers), on the shared loads, plans and epilogue.
//
//   tile route    qf_quantize_rows_kernel (one wave per row) reads X once: it writes the int8 image of A into the workspace, leading
//                 dimension r16(K) -- every chunk inside K is one aligned 16-byte load of the GEMM --, and the row sums of the flipped
//                 image, which ql_sum_rows_kernel would otherwise read the image again for.  Then the tile GEMM on the image and, for
//                 a split K, the reduce, both ending in the dequantizing epilogue.  The column sums of B are the byte route's kernels.
//   decode route  no prologue: the three kernels quantize their slice of X on the way into LDS (QA).  Every workgroup re-quantizes
//                 its slice: 4 chunks = 64 divisions a thread at the 16-row tier, against a B stream of 16 ... 64 KiB a workgroup.
//                 LDS, row sums, column sums, the streaming of B, the plan and the slabs are those of the byte route.
// The new kernels take QlArgs / QdArgs as they are: the function's x_scale / x_zero_point are the product's a_scale / a_zero_point and
// its out_scale / out_zero_point the product's y_scale / y_zero_point, so no argument is added and no kernarg offset moves.
#include "qlinear_decode_body.hpp"
#include "qlinear_tile.hpp"

#include "../../include/oq_hip_qlinear_function.h"

namespace oq {
namespace {

// ---- tile route
// Q[row, k] = the quantized X[row, k] for k < K (raw bytes of A's type; past K up to ldq the flip's byte), sums[row] = the sum over
// k of the flipped bytes read as int8 -- what ql_sum_rows_kernel gives on Q.  One wave per row, a lane takes every 64th 16-chunk.
__global__ __launch_bounds__(kThreads) void qf_quantize_rows_kernel(const QlArgs p, const float* X, int64_t ldx, int32_t x_vec, uint8_t* Q,
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
        for (int j = 0; j < 4; ++j) s = dot4(v[j] ^ p.a_flip, kOnes, s);            // past K: the flip's byte, a zero after the flip
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s), off, kWave));
    if (sums && lane == 0) sums[row] = static_cast<int32_t>(s);
}

template <int MT, int LAYOUT>
__global__ __launch_bounds__(kThreads, 2) void qf_gemm_kernel(const QlArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[ql_gemm_lds_bytes(MT)];
    ql_gemm_body<MT, LAYOUT, kEpDequantized>(p, lds);
}

__global__ __launch_bounds__(kThreads) void qf_reduce_kernel(const QlArgs p, const int splits) { ql_reduce_body<kEpDequantized>(p, splits); }

__global__ __launch_bounds__(kThreads) void qf_sum_rows_kernel(const uint8_t* X, int64_t rows, int64_t K, int64_t ld, uint32_t ubias, int32_t vec,
                                                               int32_t* sums) {
    ql_sum_rows_body(X, rows, K, ld, ubias, vec, sums);
}

__global__ __launch_bounds__(kThreads) void qf_sum_cols_kernel(const uint8_t* X, int64_t K, int64_t N, int64_t ld, uint32_t ubias, int32_t vec,
                                                               int32_t* sums, int64_t stride) {
    __shared__ uint32_t part[16][64];
    ql_sum_cols_body(X, K, N, ld, ubias, vec, sums, stride, part);
}

// ---- decode route
template <int MT, bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void qf_decode_nk_kernel(const QdArgs p) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_a[MT * (kQlDecodeSlice / 4)];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];
    ql_decode_nk_body<MT, CS, true, true>(p, lds_a, lds_rs);
}

template <bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void qf_decode_nk_mma_kernel(const QdArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_a[kQlDecodeMaxRows * kMmaRow];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];
    ql_decode_nk_mma_body<CS, true, true>(p, lds_a, lds_rs);
}

template <int MT, bool CS>
__global__ __launch_bounds__(kQlDecodeThreads) void qf_decode_kn_kernel(const QdArgs p) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[ql_decode_kn_lds_dwords(MT, CS)];
    __shared__ uint32_t lds_rs[kQlDecodeMaxRows];
    ql_decode_kn_body<MT, CS, true, true>(p, lds, lds_rs);
}

__global__ __launch_bounds__(kQlDecodeThreads) void qf_decode_reduce_kernel(const QdArgs p) { ql_decode_reduce_body<true>(p); }

// ---- host
struct FunctionPlan : Plan {      // and the workspace: include/oq_hip_qlinear_function.h, `workspace`: Q ahead of R, C, S
    uint8_t* image;               // [M, ldq] the quantized A
    int64_t ldq;                  // K rounded up to 16
};

FunctionPlan make_function_plan(int64_t M, int64_t K, int64_t N, Workspace& ws) {
    const int64_t ldq = ceil_div(K, 16) * 16;
    uint8_t* const image = ws.take<uint8_t>(static_cast<size_t>(M) * static_cast<size_t>(ldq));
    FunctionPlan pl{make_plan(M, K, N, ws)};
    pl.image = image, pl.ldq = ldq;
    return pl;
}

// what both entry points require of a call: call_ok's checks in call_ok's words, with `y_type` in the place of `out` and fp32 A and Y
int32_t function_ok(const char* fn, int64_t max_rows, const float* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale,
                    const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale, const int32_t* C,
                    const float* y_scale, int32_t flags, int32_t y_type, const float* Y, int64_t ldy) {
    OQ_REQUIRE(A && B && Y, OQ_ERR_INVALID_ARGUMENT, "%s: null pointer (A, B and Y are required)", fn);
    OQ_REQUIRE(type_ok(y_type), OQ_ERR_INVALID_ARGUMENT, "%s: unknown y_type %d", fn, y_type);
    const int32_t st = call_ok(fn, kMaxExtent, A, a_type, M, K, lda, a_scale, B, b_type, b_layout, N, ldb, b_scale, C, y_scale, flags,
                               y_type == OQ_QL_I8 ? OQ_QL_OUT_I8 : OQ_QL_OUT_U8, Y, ldy);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(M <= max_rows, OQ_ERR_UNSUPPORTED, "%s: M = %lld rows (the decode route takes 1 ... %lld; oq_qlinear_function is the route)", fn,
               (long long)M, (long long)max_rows);
    OQ_REQUIRE(aligned_to(A, 4) && aligned_to(Y, 4), OQ_ERR_INVALID_ARGUMENT, "%s: A and Y must be aligned to their element (fp32)", fn);
    return OQ_OK;
}

template <int LAYOUT>
void launch_gemm(const QlArgs& p, const Plan& pl, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
    with_row_tiles(pl, [&](auto mt) { qf_gemm_kernel<decltype(mt)::value, LAYOUT><<<grid, kThreads, 0, s>>>(p); });
}

template <bool CS>
void launch_decode(const QdArgs& p, const QdPlan& pl, bool kn, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(pl.grid);
    if (mma_route(p, pl, kn)) {
        qf_decode_nk_mma_kernel<CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
        return;
    }
    with_decode_tier(pl.tier, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        if (kn) qf_decode_kn_kernel<MT, CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
        else qf_decode_nk_kernel<MT, CS><<<grid, kQlDecodeThreads, 0, s>>>(p);
    });
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qlinear_function_extension_version(void) { return OQ_QLINEAR_FUNCTION_EXTENSION_VERSION; }

size_t oq_qlinear_function_workspace_bytes(int64_t M, int64_t K, int64_t N) {
    if (!shape_ok(M, K, N)) {
        set_error("oq_qlinear_function_workspace_bytes: M=%lld K=%lld N=%lld outside the bounds", (long long)M, (long long)K, (long long)N);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_function_plan(M, K, N, ws);
    return ws.total();
}

int32_t oq_qlinear_function(const float* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale, const void* a_zero_point,
                            const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale, const void* b_zero_point,
                            int32_t b_per_column, const int32_t* C, const float* y_scale, const void* y_zero_point, int32_t flags, int32_t y_type,
                            float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qlinear_function";
    int32_t st = function_ok(fn, kMaxExtent, A, a_type, M, K, lda, a_scale, B, b_type, b_layout, N, ldb, b_scale, C, y_scale, flags, y_type, Y, ldy);
    if (st != OQ_OK) return st;
    const bool kn = b_layout == OQ_QL_KN;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const FunctionPlan pl = make_function_plan(M, K, N, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    QlArgs p{};      // the product's operand A is the image: bytes of a_type, rows 16-byte aligned
    fill_operands(p, pl.image, a_type, M, K, pl.ldq, a_scale, a_zero_point, B, b_type, b_layout, N, ldb, b_scale, b_zero_point, b_per_column, C,
                  y_scale, y_zero_point, y_type == OQ_QL_I8 ? OQ_QL_OUT_I8 : OQ_QL_OUT_U8, Y, ldy);
    p.tiles_m = static_cast<uint32_t>(pl.tiles_m), p.steps_per_split = static_cast<uint32_t>(pl.steps_per_split);
    int32_t* rowsum = sum_needed(p.b_signed, b_zero_point) ? pl.rowsum : nullptr;
    int32_t* colsum = sum_needed(p.a_signed, a_zero_point) ? pl.colsum : nullptr;
    p.rowsum = rowsum, p.colsum = colsum;
    p.colsum_slices = kn ? kColSlices : 1, p.colsum_stride = pl.colsum_stride;
    p.slab = pl.slab;

    constexpr int kRowsPerBlock = kThreads / kWave;
    qf_quantize_rows_kernel<<<static_cast<unsigned>(ceil_div(M, kRowsPerBlock)), kThreads, 0, s>>>(p, A, lda, aligned_to(A, 16) && lda % 4 == 0, pl.image,
                                                                                                 rowsum);
    st = check_launch("qf_quantize_rows_kernel");
    if (st != OQ_OK) return st;
    if (colsum) {      // over x ^ ubias read as an unsigned byte, minus 128: ubias flips a SIGNED operand (qlinear_gemm.hip)
        const uint32_t b_ubias = p.b_flip ^ 0x80808080u;
        const int32_t vec4 = aligned_to(B, 4) && ldb % 4 == 0;
        if (kn) qf_sum_cols_kernel<<<dim3(static_cast<unsigned>(ceil_div(N, 64)), kColSlices), kThreads, 0, s>>>(p.B, K, N, ldb, b_ubias, vec4, colsum, p.colsum_stride);
        else qf_sum_rows_kernel<<<static_cast<unsigned>(ceil_div(N, kRowsPerBlock)), kThreads, 0, s>>>(p.B, N, K, ldb, b_ubias, vec4, colsum);
        st = check_launch(kn ? "qf_sum_cols_kernel" : "qf_sum_rows_kernel");
        if (st != OQ_OK) return st;
    }
    if (kn) launch_gemm<OQ_QL_KN>(p, pl, s);
    else launch_gemm<OQ_QL_NK>(p, pl, s);
    st = check_launch("qf_gemm_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    qf_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kThreads)), kThreads, 0, s>>>(p, static_cast<int>(pl.splits));
    return check_launch("qf_reduce_kernel");
}

size_t oq_qlinear_function_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t b_layout) {
    if (!shape_ok(M, K, N) || M > kQlDecodeMaxRows || !layout_ok(b_layout)) {
        set_error("oq_qlinear_function_decode_workspace_bytes: M=%lld K=%lld N=%lld b_layout=%d outside the bounds of the decode route", (long long)M,
                  (long long)K, (long long)N, b_layout);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_plan(M, K, N, b_layout, ws);
    return ws.total();
}

int32_t oq_qlinear_function_decode(const float* A, int32_t a_type, int64_t M, int64_t K, int64_t lda, const float* a_scale, const void* a_zero_point,
                                   const void* B, int32_t b_type, int32_t b_layout, int64_t N, int64_t ldb, const float* b_scale,
                                   const void* b_zero_point, int32_t b_per_column, const int32_t* C, const float* y_scale, const void* y_zero_point,
                                   int32_t flags, int32_t y_type, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qlinear_function_decode";
    int32_t st = function_ok(fn, kQlDecodeMaxRows, A, a_type, M, K, lda, a_scale, B, b_type, b_layout, N, ldb, b_scale, C, y_scale, flags, y_type, Y,
                             ldy);
    if (st != OQ_OK) return st;
    const bool kn = b_layout == OQ_QL_KN;
    Workspace ws(workspace, workspace_bytes, /* aligned_base */ true);
    const QdPlan pl = make_plan(M, K, N, b_layout, ws);
    OQ_REQUIRE(ws.total() == 0 || ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    QdArgs p{};      // p.A points at fp32 rows, lda counts floats (stage_a16<QA>)
    fill_operands(p, A, a_type, M, K, lda, a_scale, a_zero_point, B, b_type, b_layout, N, ldb, b_scale, b_zero_point, b_per_column, C, y_scale,
                  y_zero_point, y_type == OQ_QL_I8 ? OQ_QL_OUT_I8 : OQ_QL_OUT_U8, Y, ldy);
    p.a_vec = aligned_to(A, 16) && lda % 4 == 0;
    p.slice = static_cast<uint32_t>(pl.slice), p.splits = static_cast<uint32_t>(pl.splits), p.cols_per_block = static_cast<uint32_t>(pl.cols_per_block);
    p.slab = pl.slab;
    p.need_rowsum = sum_needed(p.b_signed, b_zero_point);
    if (sum_needed(p.a_signed, a_zero_point)) launch_decode<true>(p, pl, kn, s);
    else launch_decode<false>(p, pl, kn, s);
    st = check_launch(kn ? "qf_decode_kn_kernel" : "qf_decode_nk_kernel");
    if (st != OQ_OK || pl.splits == 1) return st;
    qf_decode_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kQlDecodeThreads)), kQlDecodeThreads, 0, s>>>(p);
    return check_launch("qf_decode_reduce_kernel");
}

}  // extern "C"
