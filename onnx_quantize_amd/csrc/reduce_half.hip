// C1 (calibration min/max, minmax.py:40-64) and S1 (absmax, smooth_quant.py:62-74) on fp16 / bf16 activations for gfx950
// (include/oq_hip_half.h, entries C1 / S1): the 2-byte tensor is read as it is, once, never cast to an fp32 copy.
//
// Min, max and |x| of fp16 / bf16 values are exact, so every result is that of reduce.hip's fp32 kernels on the upcast
// tensor, bit for bit.  The structure is reduce.hip's: 16-byte non-temporal loads (8 elements each), eight of them in flight
// per lane, [head | 16-byte body | tail] peeling for a base that is only 2-byte aligned, butterfly + LDS folds, and a second
// stage that applies minmax.py:50-64 to the fp32 state {min, max, seen, -} in device memory.
//
// fp16 stays packed in the body: __builtin_elementwise_minimum / maximum on two halves are v_pk_minimum3_f16 /
// v_pk_maximum3_f16 (IEEE 754-2019: NaN propagates, -0 < +0, subnormals are values), half an instruction per element for
// both extrema.  bf16 has no packed compare: a shift / a mask widens it exactly and v_minimum3_f32 / v_maximum3_f32 fold it,
// two instructions per element.  A CU issues 64 lane-operations per cycle and HBM feeds it about 6.5 half elements per cycle,
// so both stay far below the issue rate.
#include "half_elem.hpp"

namespace oq {

constexpr int kHalfBlock = 512;       // 8 waves
constexpr int kHalfMaxBlocks = 2048;  // <= 256 CUs x 8 blocks (cdna_hip_programming.md Guideline 11)
constexpr int kHalfDepth = 8;         // 16-byte loads in flight per lane, as reduce.hip's stream_minmax

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) u32x4 global_u32x4;

// Running (min, max) of one lane over 16-byte words of eight elements.
template <typename E> struct HalfRange;

template <> struct HalfRange<ElemF16> {   // fp16: two packed lanes per extremum, joined at the end
    h16x2 mn, mx;
    __device__ __forceinline__ HalfRange() {
        const _Float16 inf = __builtin_bit_cast(_Float16, static_cast<uint16_t>(0x7C00)), ninf = __builtin_bit_cast(_Float16, static_cast<uint16_t>(0xFC00));
        mn = h16x2{inf, inf};
        mx = h16x2{ninf, ninf};
    }
    // by value: __builtin_bit_cast applied to `a.x` itself reads element 0 whichever element is named
    static __device__ __forceinline__ h16x2 pair(uint32_t w) { return __builtin_bit_cast(h16x2, w); }
    __device__ __forceinline__ void fold(const u32x4 a) {
        const h16x2 v0 = pair(a.x), v1 = pair(a.y), v2 = pair(a.z), v3 = pair(a.w);
        mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mn, v0), v1);
        mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mn, v2), v3);
        mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mx, v0), v1);
        mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mx, v2), v3);
    }
    __device__ __forceinline__ float lo() const { return nmin(static_cast<float>(mn.x), static_cast<float>(mn.y)); }
    __device__ __forceinline__ float hi() const { return nmax(static_cast<float>(mx.x), static_cast<float>(mx.y)); }
};

template <> struct HalfRange<ElemBF16> {   // bf16: widened by a shift (low half) / a mask (high half), folded in fp32
    float mn, mx;
    __device__ __forceinline__ HalfRange() : mn(INFINITY), mx(-INFINITY) {}
    __device__ __forceinline__ void word(uint32_t w) {
        const float a = __uint_as_float(w << 16), b = __uint_as_float(w & 0xFFFF0000u);
        mn = nmin(nmin(mn, a), b);
        mx = nmax(nmax(mx, a), b);
    }
    __device__ __forceinline__ void fold(const u32x4 a) { word(a.x); word(a.y); word(a.z); word(a.w); }
    __device__ __forceinline__ float lo() const { return mn; }
    __device__ __forceinline__ float hi() const { return mx; }
};

__device__ __forceinline__ void block_minmax_f32(float& mn, float& mx, float* s_mn, float* s_mx) {
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w) {
            mn = nmin(mn, s_mn[w]);
            mx = nmax(mx, s_mx[w]);
        }
    }
}

// One block's share of a flat 2-byte array: grid-stride over the 16-byte body with kHalfDepth loads in flight, then the head
// (< 8 elements in front of the first 16-byte boundary) and the tail (< 8 elements) one element per lane.
template <typename E>
__device__ __forceinline__ void half_range(const uint16_t* x, int64_t count, int64_t tid, int64_t stride, float& mn, float& mx) {
    int64_t vec_off = static_cast<int64_t>(((16 - reinterpret_cast<uintptr_t>(x) % 16) % 16) / 2);
    if (vec_off > count) vec_off = count;
    const int64_t nvec = (count - vec_off) / 8;
    // a pointer that came out of a descriptor is a generic one to the compiler: say that it is global memory (global_load, not flat_load)
    const global_u32x4* xv = (const global_u32x4*)(x + vec_off);
    HalfRange<E> acc;
    int64_t i = tid;
    for (; i + (kHalfDepth - 1) * stride < nvec; i += kHalfDepth * stride) {
        u32x4 a[kHalfDepth];
#pragma unroll
        for (int u = 0; u < kHalfDepth; ++u) a[u] = __builtin_nontemporal_load(xv + i + u * stride);
#pragma unroll
        for (int u = 0; u < kHalfDepth; ++u) acc.fold(a[u]);
    }
    for (; i < nvec; i += stride) acc.fold(__builtin_nontemporal_load(xv + i));
    mn = acc.lo();
    mx = acc.hi();
    for (int64_t j = tid; j < vec_off; j += stride) { const float v = E::one(x[j]); mn = nmin(mn, v); mx = nmax(mx, v); }
    for (int64_t j = vec_off + nvec * 8 + tid; j < count; j += stride) { const float v = E::one(x[j]); mn = nmin(mn, v); mx = nmax(mx, v); }
}

struct HalfDesc {   // device-resident, 24 bytes per tensor (oq_hip.h: oq_minmax_desc, x read as a 2-byte pointer)
    const uint16_t* x;
    int64_t count;
    float* state;
};

// Stage 1.  desc == nullptr: the one tensor (x, count), blockIdx.x = slice.  Otherwise blockIdx.y = tensor of the list.
template <typename E>
__global__ __launch_bounds__(kHalfBlock) void minmax_half_partial(const HalfDesc* desc, const uint16_t* x, int64_t count,
                                                                  float* partial /* [tensors][gridDim.x][2] */) {
    __shared__ float s_mn[kHalfBlock / 64], s_mx[kHalfBlock / 64];
    if (desc != nullptr) {
        const HalfDesc d = desc[blockIdx.y];
        x = d.x;
        count = d.count;
    }
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    float mn, mx;
    half_range<E>(x, count, tid, stride, mn, mx);
    block_minmax_f32(mn, mx, s_mn, s_mx);
    if (threadIdx.x == 0) {
        float* o = partial + (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * 2;
        o[0] = mn;
        o[1] = mx;
    }
}

// Stage 2, one block per tensor: fold its slices and apply minmax.py:50-64 to its fp32 state (reduce.hip: minmax_update).
__global__ __launch_bounds__(kHalfBlock) void minmax_half_update(const HalfDesc* desc, float* state, const float* partial, int slices,
                                                                 double momentum) {
    __shared__ float s_mn[kHalfBlock / 64], s_mx[kHalfBlock / 64];
    const float* p = partial + static_cast<int64_t>(blockIdx.x) * slices * 2;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < slices; i += blockDim.x) {
        mn = nmin(mn, p[2 * i]);
        mx = nmax(mx, p[2 * i + 1]);
    }
    block_minmax_f32(mn, mx, s_mn, s_mx);
    if (threadIdx.x != 0) return;
    if (desc != nullptr) state = desc[blockIdx.x].state;
    if (state[2] == 0.0f) {            // minmax.py:50-51 first sight
        state[0] = mn;
        state[1] = mx;
        state[2] = 1.0f;
    } else if (momentum > 0.0) {       // minmax.py:53-60 EMA; products rounded separately (no FMA)
        const float m = static_cast<float>(momentum), om = static_cast<float>(1.0 - momentum);
        state[0] = m * state[0] + om * mn;
        state[1] = m * state[1] + om * mx;
    } else {                           // minmax.py:63-64
        state[0] = nmin(state[0], mn);
        state[1] = nmax(state[1], mx);
    }
}

static int half_many_slices(int64_t n) {   // ~4096 blocks in total, 4..64 slices per tensor (reduce.hip: many_slices)
    int64_t s = 4096 / (n > 0 ? n : 1);
    if (s < 4) s = 4;
    if (s > 64) s = 64;
    return static_cast<int>(s);
}

// ------------------------------------------------------------------------------------- absmax
constexpr int kHalfAbsChunkRows = 128;   // rows per block: 8 waves x 16 rows
constexpr int kHalfAbsTileCols = 512;    // columns per block: 64 lanes x 8 elements

template <typename E>
__device__ __forceinline__ void absmax8(float (&mx)[8], const u32x4 a) {
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mx[2 * i] = nmax(mx[2 * i], fabsf(E::one(static_cast<uint16_t>(w[i] & 0xFFFFu))));
        mx[2 * i + 1] = nmax(mx[2 * i + 1], fabsf(E::one(static_cast<uint16_t>(w[i] >> 16))));
    }
}

// vec8: every row starts on a 16-byte boundary and C % 8 == 0 -- lane l owns columns col0 + 8 l .. + 7 (one 16-byte load per
// row).  Otherwise lane l owns columns col0 + 64 i + l, i = 0..7, read one element at a time.
template <typename E>
__global__ __launch_bounds__(512) void absmax_half_cols_partial(const uint16_t* x, int64_t R, int64_t C, int64_t ldx, bool vec8,
                                                                float* partial, uint32_t ncol_tiles) {
    __shared__ float s_mx[8][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col_tile = blockIdx.x % ncol_tiles, chunk = blockIdx.x / ncol_tiles;
    const int64_t row0 = static_cast<int64_t>(chunk) * kHalfAbsChunkRows + wave * 16;
    const int64_t col0 = static_cast<int64_t>(col_tile) * kHalfAbsTileCols;
    float mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (vec8) {
        const int64_t c = col0 + lane * 8;
        if (c < C) {
            u32x4 t[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                t[r] = (row0 + r < R) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + (row0 + r) * ldx + c)) : u32x4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 16; ++r) absmax8<E>(mx, t[r]);
        }
    } else {
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t c = col0 + i * 64 + lane;
                if (c < C && row0 + r < R) mx[i] = nmax(mx[i], fabsf(E::one(x[(row0 + r) * ldx + c])));
            }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s_mx[wave][i][lane] = mx[i];
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 8; ++w)
#pragma unroll
        for (int i = 0; i < 8; ++i) mx[i] = nmax(mx[i], s_mx[w][i][lane]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t c = vec8 ? col0 + lane * 8 + i : col0 + i * 64 + lane;
        if (c < C) partial[static_cast<int64_t>(chunk) * C + c] = mx[i];
    }
}

__global__ void absmax_half_cols_finalize(const float* partial, int64_t chunks, int64_t C, float* out) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float m = 0.f;
    for (int64_t k = 0; k < chunks; ++k) m = nmax(m, partial[k * C + c]);
    out[c] = m;
}

// one wave per row
template <typename E>
__global__ __launch_bounds__(256) void absmax_half_rows(const uint16_t* x, int64_t R, int64_t C, int64_t ldx, bool vec8, float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const uint16_t* row = x + r * ldx;
    float m = 0.f;
    if (vec8) {
        float mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int64_t c = lane * 8; c < C; c += 512) absmax8<E>(mx, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + c)));
        m = nmax(nmax(nmax(mx[0], mx[1]), nmax(mx[2], mx[3])), nmax(nmax(mx[4], mx[5]), nmax(mx[6], mx[7])));
    } else {
        for (int64_t c = lane; c < C; c += 64) m = nmax(m, fabsf(E::one(row[c])));
    }
    m = wave_max(m);
    if (lane == 0) out[r] = m;
}

}  // namespace oq

extern "C" {

using namespace oq;

// The workspaces of this file are single arrays of partial results, used from the caller's pointer on: one formula each, shared
// by the query and the entry point.  (The `+ 256` of two queries is room the entry points never asked for; the header states it.)
constexpr size_t kMinmaxHalfPartialBytes = static_cast<size_t>(kHalfMaxBlocks) * 2 * sizeof(float);      // one (min, max) per block
static size_t absmax_half_partial_bytes(int64_t R, int64_t C) { return static_cast<size_t>(ceil_div(R, kHalfAbsChunkRows) * C) * sizeof(float); }

size_t oq_minmax_half_workspace_bytes(int64_t count) {
    if (!count_ok(count)) return 0;
    return kMinmaxHalfPartialBytes;
}

int32_t oq_minmax_collect_h16(const void* x, int32_t xtype, int64_t count, float* state, double momentum, void* workspace,
                              size_t workspace_bytes, void* stream) {
    // every check before any arithmetic on an extent and before any HIP call
    int32_t st = half_operand_ok("oq_minmax_collect_h16", "x", xtype, x);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(x != nullptr && state != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_h16: null x / state");
    OQ_REQUIRE(aligned_to(state, 4), OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_h16: state must be 4-byte aligned");
    OQ_REQUIRE(count_ok(count), OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_h16: bad count=%lld (1 <= count <= 2^40)", (long long)count);
    OQ_REQUIRE(momentum >= 0.0 && momentum < 1.0, OQ_ERR_INVALID_ARGUMENT, "Momentum must be in the range [0, 1) (momentum=%g).", momentum);
    const size_t need = kMinmaxHalfPartialBytes;
    OQ_REQUIRE(workspace != nullptr && workspace_bytes >= need, OQ_ERR_WORKSPACE, "oq_minmax_collect_h16: workspace of %zu bytes needed, %zu given",
               need, workspace_bytes);
    // every block gets at least one eight-deep round of its 512 lanes (32768 elements) before a second block is started
    int64_t nblocks = count / (static_cast<int64_t>(kHalfBlock) * kHalfDepth * 8);
    if (nblocks > kHalfMaxBlocks) nblocks = kHalfMaxBlocks;
    if (nblocks < 1) nblocks = 1;
    hipStream_t s = as_stream(stream);
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    float* partial = static_cast<float*>(workspace);
    const dim3 grid(static_cast<uint32_t>(nblocks));
    with_half_elem(xtype, [&](auto e) { hipLaunchKernelGGL(minmax_half_partial<decltype(e)>, grid, dim3(kHalfBlock), 0, s, nullptr, xh, count, partial); });
    st = check_launch("minmax_half_partial");
    if (st != OQ_OK) return st;
    hipLaunchKernelGGL(minmax_half_update, dim3(1), dim3(kHalfBlock), 0, s, nullptr, state, partial, static_cast<int>(nblocks), momentum);
    return check_launch("minmax_half_update");
}

size_t oq_minmax_many_half_workspace_bytes(int64_t n) {
    if (n <= 0 || n > 65535) return 0;
    return static_cast<size_t>(n) * half_many_slices(n) * 2 * sizeof(float) + 256;
}

int32_t oq_minmax_collect_many_h16(const void* desc, int64_t n, int32_t xtype, double momentum, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    static_assert(sizeof(HalfDesc) == sizeof(oq_minmax_desc), "the descriptor of oq_hip.h");
    int32_t st = half_operand_ok("oq_minmax_collect_many_h16", "x", xtype, nullptr);   // the tensors' pointers: device memory, not looked at
    if (st != OQ_OK) return st;
    OQ_REQUIRE(desc != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_many_h16: null desc");
    OQ_REQUIRE(aligned_to(desc, 8), OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_many_h16: desc must be 8-byte aligned");
    OQ_REQUIRE(n > 0 && n <= 65535, OQ_ERR_INVALID_ARGUMENT, "oq_minmax_collect_many_h16: bad n=%lld (1 <= n <= 65535)", (long long)n);
    OQ_REQUIRE(momentum >= 0.0 && momentum < 1.0, OQ_ERR_INVALID_ARGUMENT, "Momentum must be in the range [0, 1) (momentum=%g).", momentum);
    const size_t need = oq_minmax_many_half_workspace_bytes(n);
    OQ_REQUIRE(workspace != nullptr && workspace_bytes >= need, OQ_ERR_WORKSPACE,
               "oq_minmax_collect_many_h16: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    const int slices = half_many_slices(n);
    hipStream_t s = as_stream(stream);
    const HalfDesc* d = static_cast<const HalfDesc*>(desc);
    float* partial = static_cast<float*>(workspace);
    const dim3 grid(static_cast<uint32_t>(slices), static_cast<uint32_t>(n));
    with_half_elem(xtype, [&](auto e) { hipLaunchKernelGGL(minmax_half_partial<decltype(e)>, grid, dim3(kHalfBlock), 0, s, d, nullptr, int64_t{0}, partial); });
    st = check_launch("minmax_half_partial");
    if (st != OQ_OK) return st;
    hipLaunchKernelGGL(minmax_half_update, dim3(static_cast<uint32_t>(n)), dim3(kHalfBlock), 0, s, d, nullptr, partial, slices, momentum);
    return check_launch("minmax_half_update");
}

size_t oq_absmax_half_workspace_bytes(int64_t R, int64_t C, int32_t transposed) {
    if (!matrix_ok(R, C, C)) return 0;
    if (transposed) return 256;
    return absmax_half_partial_bytes(R, C) + 256;
}

int32_t oq_absmax_h16(const void* x, int32_t xtype, int64_t R, int64_t C, int64_t ldx, int32_t transposed, float* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    int32_t st = half_operand_ok("oq_absmax_h16", "x", xtype, x);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(x != nullptr && out != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_absmax_h16: null x / out");
    OQ_REQUIRE(aligned_to(out, 4), OQ_ERR_INVALID_ARGUMENT, "oq_absmax_h16: out must be 4-byte aligned");
    OQ_REQUIRE(matrix_ok(R, C, ldx), OQ_ERR_INVALID_ARGUMENT, "oq_absmax_h16: bad shape R=%lld C=%lld ldx=%lld", (long long)R, (long long)C,
               (long long)ldx);
    const bool vec8 = (C % 8 == 0) && (ldx % 8 == 0) && aligned_to(x, 16);
    hipStream_t s = as_stream(stream);
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (transposed) {
        const dim3 grid(static_cast<uint32_t>(ceil_div(R, 4)));
        with_half_elem(xtype, [&](auto e) { hipLaunchKernelGGL(absmax_half_rows<decltype(e)>, grid, dim3(256), 0, s, xh, R, C, ldx, vec8, out); });
        return check_launch("absmax_half_rows");
    }
    const int64_t chunks = ceil_div(R, kHalfAbsChunkRows);
    const size_t need = absmax_half_partial_bytes(R, C);
    OQ_REQUIRE(workspace != nullptr && workspace_bytes >= need, OQ_ERR_WORKSPACE, "oq_absmax_h16: workspace of %zu bytes needed, %zu given", need,
               workspace_bytes);
    OQ_REQUIRE(aligned_to(workspace, 4), OQ_ERR_INVALID_ARGUMENT, "oq_absmax_h16: workspace must be 4-byte aligned");
    const int64_t ncol_tiles = ceil_div(C, kHalfAbsTileCols);   // x chunks < 2^26: R * ldx <= 2^40, 128 x 512 elements per block
    float* partial = static_cast<float*>(workspace);
    const dim3 grid(static_cast<uint32_t>(ncol_tiles * chunks));
    with_half_elem(xtype, [&](auto e) {
        hipLaunchKernelGGL(absmax_half_cols_partial<decltype(e)>, grid, dim3(512), 0, s, xh, R, C, ldx, vec8, partial, static_cast<uint32_t>(ncol_tiles));
    });
    st = check_launch("absmax_half_cols_partial");
    if (st != OQ_OK) return st;
    hipLaunchKernelGGL(absmax_half_cols_finalize, dim3(static_cast<uint32_t>(ceil_div(C, 256))), dim3(256), 0, s, partial, chunks, C, out);
    return check_launch("absmax_half_cols_finalize");
}

}  // extern "C"
