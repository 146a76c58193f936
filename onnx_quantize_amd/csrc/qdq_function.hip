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
// dynamic input.  New with this route: the min / max pass over X, the one-workgroup kernel that turns its pairs into parameters, and
// the launch that finishes a dynamic output.  They, the prologue, the reduce and the plan are in qdq_function_parts.hpp, which
// qdq_function_packed4.hip shares; this file keeps the product and W's column sums.  The launches of each variant: the header.
#include "qdq_function_parts.hpp"

namespace oq {
namespace {

constexpr int64_t kMaxK = 33025;            // 255 * 255 * K <= 2^31 - 1: no int32 sum can wrap

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
    QdqArgs p{};
    const float* const quant_scale = fill_qdq_args(p, pl, M, K, x_mode, x_type, x_scale, x_zero_point, W, wtype == OQ_INT8 ? OQ_QL_I8 : OQ_QL_U8, N, ldw,
                                                   w_scale, w_zero_point, granularity == OQ_CHANNEL, B, b_scale, b_zero_point, out_mode, out_type,
                                                   out_scale, out_zero_point, Y, ldy);
    return run_qdq_function(p, pl, static_cast<const float*>(X), lda, quant_scale, Y, ldy, s, [&]() -> int32_t {
        if (p.colsum) {      // over w ^ ubias read as an unsigned byte, minus 128: ubias flips a SIGNED operand (qlinear_gemm.hip)
            qq_sum_cols_kernel<<<dim3(static_cast<unsigned>(ceil_div(N, 64)), kColSlices), kThreads, 0, s>>>(
                p.B, K, N, ldw, p.b_flip ^ 0x80808080u, aligned_to(W, 4) && ldw % 4 == 0, pl.colsum, p.colsum_stride);
            const int32_t st = check_launch("qq_sum_cols_kernel");
            if (st != OQ_OK) return st;
        }
        const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
        with_row_tiles(pl, [&](auto mt) { qq_gemm_kernel<decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
        return check_launch("qq_gemm_kernel");
    });
}

}  // extern "C"
