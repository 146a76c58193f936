// What the two entry points of a QDQ function with quantized activations share around their product (qdq_function.hip,
// include/oq_hip_qdq_function.h; qdq_function_packed4.hip, include/oq_hip_qdq_function_packed4.h): the argument block of the epilogue
// kEpQdqFunction, the min / max pass over X and the one-workgroup kernel that turns its pairs into parameters (a dynamic input), the
// quantizing prologue, the split-K reduce, the launch that finishes a dynamic output, and the plan with the workspace layout.  One
// text: each file that includes it gets these kernels with its own build flags, as with the kernels of nbits_tile.hpp.  The product
// kernel and the column sums of W are each file's own.
#pragma once

#include "qlinear_tile.hpp"

#include "../../include/oq_hip_qdq_function.h"

namespace oq {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// ---- the slabs of a split K
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

// The argument block of a call that its entry point has let through.  The product's operand A is the image: bytes of x_type (uint8
// for a dynamic input), rows 16-byte aligned; out F32: col_terms forms the scale.  B: the operand as the product kernel reads it,
// `b_type` / `b_zero_point` what the EPILOGUE is to correct for.  A dynamic input: the quantizer divides by `safe`, the product scales
// by `scale`, the zero point is the low byte of the block's dword.  Returns what the quantizer divides by.
template <class P>
const float* fill_qdq_args(P& p, const QdqFunctionPlan& pl, int64_t M, int64_t K, int32_t x_mode, int32_t x_type, const float* x_scale,
                           const void* x_zero_point, const void* W, int32_t b_type, int64_t N, int64_t ldw, const float* w_scale,
                           const void* b_zero_point, bool per_column, const int32_t* B, const float* b_scale, const int32_t* bias_zero_point,
                           int32_t out_mode, int32_t out_type, const float* out_scale, const void* out_zero_point, float* Y, int64_t ldy) {
    const bool dynamic_x = x_mode == OQ_QDQ_DYNAMIC;
    const int32_t a_type = dynamic_x ? OQ_QL_U8 : x_type;
    const float* const prod_scale = dynamic_x ? &pl.params->scale : x_scale;
    const void* const a_zp = dynamic_x ? static_cast<const void*>(&pl.params->zp) : x_zero_point;
    fill_operands(p, pl.image, a_type, M, K, pl.ldq, prod_scale, a_zp, W, b_type, OQ_QL_KN, N, ldw, w_scale, b_zero_point, per_column, nullptr,
                  out_scale, out_zero_point, OQ_QL_OUT_F32, Y, ldy);
    p.tiles_m = static_cast<uint32_t>(pl.tiles_m), p.steps_per_split = static_cast<uint32_t>(pl.steps_per_split);
    p.rowsum = sum_needed(p.b_signed, b_zero_point) ? pl.rowsum : nullptr;
    p.colsum = sum_needed(p.a_signed, a_zp) ? pl.colsum : nullptr;
    p.colsum_slices = kColSlices, p.colsum_stride = pl.colsum_stride;
    p.slab = pl.slab;
    p.bias = B, p.bias_scale = b_scale, p.bias_zp = bias_zero_point;
    p.out_mode = out_mode, p.out_signed = out_mode == OQ_QDQ_STATIC && out_type == OQ_QL_I8, p.pairs = pl.out_pairs;
    return dynamic_x ? &pl.params->safe : x_scale;
}

// The launches of a call behind its argument block, which both entry points run in one order: [min / max of X, its parameters,]
// the quantizing prologue, `product` -- the caller's column sums and tile GEMM; it returns their status -- [the reduce of a split K,]
// [the finish of a dynamic output].  `q_scale`: what the quantizer divides by (fill_qdq_args).
template <class F>
int32_t run_qdq_function(const QdqArgs& p, const QdqFunctionPlan& pl, const float* x, int64_t lda, const float* q_scale, float* Y, int64_t ldy,
                         hipStream_t s, F&& product) {
    const int64_t M = p.M, N = p.N;
    const bool dynamic_x = pl.params != nullptr;
    int32_t* const rowsum = p.rowsum ? pl.rowsum : nullptr;
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
    q.a_scale = q_scale;
    qq_quantize_rows_kernel<<<static_cast<unsigned>(ceil_div(M, kWaves)), kThreads, 0, s>>>(q, x, lda, x_vec, pl.image, rowsum);
    st = check_launch("qq_quantize_rows_kernel");
    if (st != OQ_OK) return st;
    st = product();
    if (st != OQ_OK) return st;
    if (pl.splits > 1) {
        qq_reduce_kernel<<<static_cast<unsigned>(ceil_div(M * N, kThreads)), kThreads, 0, s>>>(p, static_cast<int>(pl.splits));
        st = check_launch("qq_reduce_kernel");
        if (st != OQ_OK) return st;
    }
    if (p.out_mode != OQ_QDQ_DYNAMIC) return OQ_OK;
    const int32_t y_vec = aligned_to(Y, 16) && ldy % 4 == 0 && N % 4 == 0;
    const int64_t work = y_vec ? M * (N / 4) : M * N;
    qq_finish_dynamic_kernel<<<static_cast<unsigned>(std::min<int64_t>(ceil_div(work, kThreads), 2048)), kThreads, 0, s>>>(
        Y, p.M, p.N, ldy, y_vec, pl.out_pairs, static_cast<uint32_t>(pl.out_blocks));
    return check_launch("qq_finish_dynamic_kernel");
}

}  // namespace
}  // namespace oq
