// N2s: the |x| column statistics of the AWQ / SmoothQuant searches (awq.py:47-50 sum_t |x[t, k]|, smooth_quant.py:62-69
// max_t |x[t, k]|) on LISTS of fp16 / bf16 activations for gfx950 (include/oq_hip_half.h, entry N2s): every tensor is read as it
// is, once, for both statistics, and a whole calibration batch takes two launches (partials, fold).
//
// |x| of an fp16 / bf16 value is exact in fp32, so the maximum is that of any order.  The sum is not: its order per column is
// that of oq_abs_sum_cols_f32 (awq.hip: col_abs_partial_kernel<false>, col_abs_accumulate_kernel) -- min(T, 64) row chunks of
// ceil(T / chunks) rows, fours as (a + b) + (c + d) and then single rows inside a chunk, the chunks added from 0, the result
// added to the running value -- so `abs_sum` comes out with the bits of that entry point on the upcast matrix.  Only how
// columns map to lanes differs: a lane owns 8, 4, 2 or 1 ADJACENT columns (16-, 8-, 4- or 2-byte non-temporal loads), as the
// alignment of the item's rows allows and, for small tables, as few as still fill the device with waves.  A lane keeps 8
// (16-byte) or 16 (narrower) row loads in flight: two or four of the fours, summed in row order.
//
// No block waits for another and nothing is atomic: stage 1 writes [chunk][k] partial sums and maxima, stage 2 folds them.
#include "half_elem.hpp"

namespace oq {

constexpr int kStatChunks = 64;       // awq.hip: kColChunks -- part of the sum order
constexpr int kStatBlock = 256;       // 4 waves
constexpr int64_t kStatFillLanes = 256 * 4 * 64 * 4;   // four waves on every SIMD of 256 CUs

struct StatItem {   // oq_abs_stats_item with X as a 2-byte pointer
    const uint16_t* X;
    int64_t T, K, ldx;
    float* abs_sum;
    float* absmax;
};

__host__ __device__ __forceinline__ int stat_chunks(int64_t T) { return T < kStatChunks ? static_cast<int>(T) : kStatChunks; }

// Adjacent columns per lane of one item: the widest of 8 / 4 / 2 (at most `cap`) whose loads stay aligned in every row and
// inside the row (K, ldx multiples of it, the base aligned to it), else 1.  The host sizes the grid with the same function.
__host__ __device__ __forceinline__ int stat_width(const void* X, int64_t K, int64_t ldx, int cap) {
    const uint64_t bits = static_cast<uint64_t>(K) | static_cast<uint64_t>(ldx) | (static_cast<uint64_t>(reinterpret_cast<uintptr_t>(X)) >> 1);
    for (int v = cap; v > 1; v >>= 1)
        if ((bits & static_cast<uint64_t>(v - 1)) == 0) return v;
    return 1;
}

template <typename E>
__device__ __forceinline__ float abs_widen(uint32_t b /* the element in the low 16 bits */) {
    // bf16: the shift and the sign mask on the word itself; fabsf(ElemBF16::one(..)) is the same value in 7 % more instructions
    if constexpr (std::is_same_v<E, ElemBF16>) return __uint_as_float((b << 16) & 0x7FFFFFFFu);
    else return fabsf(E::one(static_cast<uint16_t>(b)));
}

template <int V> struct StatRaw;
template <> struct StatRaw<8> { typedef u32x4 type; };
template <> struct StatRaw<4> { typedef u32x2 type; };
template <> struct StatRaw<2> { typedef uint32_t type; };
template <> struct StatRaw<1> { typedef uint16_t type; };

template <int V>
__device__ __forceinline__ typename StatRaw<V>::type stat_load(const uint16_t* p) {
    typedef typename StatRaw<V>::type raw;
    // a pointer that came out of a table is a generic one to the compiler: say that it is global memory (global_load, not flat_load)
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) raw*)p);
}

template <typename E, int V>
__device__ __forceinline__ void stat_unpack(const typename StatRaw<V>::type r, float (&a)[V]) {
    if constexpr (V == 1) {
        a[0] = abs_widen<E>(r);
    } else if constexpr (V == 2) {
        a[0] = abs_widen<E>(r & 0xFFFFu);
        a[1] = abs_widen<E>(r >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < V / 2; ++i) {
            a[2 * i] = abs_widen<E>(r[i] & 0xFFFFu);
            a[2 * i + 1] = abs_widen<E>(r[i] >> 16);
        }
    }
}

// One lane's V columns over the `rows` rows of its chunk, `x` at the chunk's first row.
template <typename E, int V, int DEPTH>
__device__ __forceinline__ void stat_lane(const uint16_t* x, int64_t ldx, int64_t rows, float* psum, float* pmax) {
    static_assert(DEPTH % 4 == 0, "whole fours");
    typedef typename StatRaw<V>::type raw;
    float s[V], m[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = m[i] = 0.f;
    auto four = [&](const raw r0, const raw r1, const raw r2, const raw r3) {
        float a[V], b[V], c[V], d[V];
        stat_unpack<E, V>(r0, a);
        stat_unpack<E, V>(r1, b);
        stat_unpack<E, V>(r2, c);
        stat_unpack<E, V>(r3, d);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            s[i] += (a[i] + b[i]) + (c[i] + d[i]);
            m[i] = nmax(nmax(m[i], a[i]), nmax(b[i], nmax(c[i], d[i])));
        }
    };
    int64_t t = 0;
    for (; t + DEPTH <= rows; t += DEPTH) {
        raw r[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) r[u] = stat_load<V>(x + (t + u) * ldx);
#pragma unroll
        for (int u = 0; u < DEPTH; u += 4) four(r[u], r[u + 1], r[u + 2], r[u + 3]);
    }
    for (; t + 4 <= rows; t += 4) {
        const raw r0 = stat_load<V>(x + t * ldx), r1 = stat_load<V>(x + (t + 1) * ldx), r2 = stat_load<V>(x + (t + 2) * ldx),
                  r3 = stat_load<V>(x + (t + 3) * ldx);
        four(r0, r1, r2, r3);
    }
    for (; t < rows; ++t) {
        float a[V];
        stat_unpack<E, V>(stat_load<V>(x + t * ldx), a);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            s[i] += a[i];
            m[i] = nmax(m[i], a[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        psum[i] = s[i];
        pmax[i] = m[i];
    }
}

// Stage 1.  blockIdx.y = item, blockIdx.x = column tile * chunks + chunk of that item (blocks past its last tile leave at once).
// partial: `slot` floats of sums [chunk][k] and `slot` floats of maxima per item.  table == nullptr: the one item `one`.
template <typename E>
__global__ __launch_bounds__(kStatBlock) void abs_stats_half_partial(const StatItem* table, const StatItem one, int cap, int64_t slot, float* partial) {
    StatItem it = one;
    if (table != nullptr) it = table[blockIdx.y];            // uniform: scalar loads
    const int chunks = stat_chunks(it.T);
    const int v = stat_width(it.X, it.K, it.ldx, cap);
    const uint32_t chunk = blockIdx.x % static_cast<uint32_t>(chunks), tile = blockIdx.x / static_cast<uint32_t>(chunks);
    const int64_t c = (static_cast<int64_t>(tile) * kStatBlock + threadIdx.x) * v;
    if (c >= it.K) return;                                   // K % v == 0: a lane's columns are inside the row or all outside
    const int64_t per = (it.T + chunks - 1) / chunks;
    const int64_t t0 = static_cast<int64_t>(chunk) * per;
    const int64_t rows = (t0 + per < it.T ? t0 + per : it.T) - t0;   // <= 0 for the chunks behind the last row: zeros, as awq.hip writes
    float* psum = partial + static_cast<int64_t>(blockIdx.y) * slot * 2 + static_cast<int64_t>(chunk) * it.K + c;
    float* pmax = psum + static_cast<int64_t>(chunks) * it.K;
    const uint16_t* x = it.X + t0 * it.ldx + c;
    switch (v) {                                             // uniform over the block
        case 8: stat_lane<E, 8, 8>(x, it.ldx, rows, psum, pmax); break;
        case 4: stat_lane<E, 4, 16>(x, it.ldx, rows, psum, pmax); break;
        case 2: stat_lane<E, 2, 16>(x, it.ldx, rows, psum, pmax); break;
        default: stat_lane<E, 1, 16>(x, it.ldx, rows, psum, pmax); break;
    }
}

// Stage 2, one lane per column: the chunks from 0 (col_abs_accumulate_kernel), then the running values.
__global__ __launch_bounds__(kStatBlock) void abs_stats_half_fold(const StatItem* table, const StatItem one, int64_t slot, const float* partial) {
    StatItem it = one;
    if (table != nullptr) it = table[blockIdx.y];
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kStatBlock + threadIdx.x;
    if (k >= it.K) return;
    const int chunks = stat_chunks(it.T);
    const float* psum = partial + static_cast<int64_t>(blockIdx.y) * slot * 2 + k;
    const float* pmax = psum + static_cast<int64_t>(chunks) * it.K;
    float acc = 0.f, m = 0.f;
    for (int c = 0; c < chunks; ++c) acc += psum[static_cast<int64_t>(c) * it.K];
    for (int c = 0; c < chunks; ++c) m = nmax(m, pmax[static_cast<int64_t>(c) * it.K]);
    typedef __attribute__((address_space(1))) float global_float;   // pointers out of a table: global memory, not flat
    global_float* sum = (global_float*)it.abs_sum + k;
    global_float* mx = (global_float*)it.absmax + k;
    *sum = *sum + acc;
    *mx = nmax(*mx, m);                                      // NaN in the running value or in the column: NaN (torch.maximum)
}

struct StatPlan {
    int64_t slot;       // floats of one statistic per item: max over the items of chunks * K
    int64_t max_k;
    int64_t lanes8;     // lanes of stage 1 if every item took 8 columns per lane
};

// The extents of the table (no pointer is looked at).  Returns the index of the first item outside the bounds, -1 if none.
static int64_t stat_plan(const oq_abs_stats_item* items, int64_t count, StatPlan* p) {
    p->slot = p->max_k = p->lanes8 = 0;
    for (int64_t i = 0; i < count; ++i) {
        const oq_abs_stats_item& it = items[i];
        if (!matrix_ok(it.T, it.K, it.ldx)) return i;
        const int64_t chunks = stat_chunks(it.T);
        if (chunks * it.K > p->slot) p->slot = chunks * it.K;
        if (it.K > p->max_k) p->max_k = it.K;
        p->lanes8 += chunks * ceil_div(it.K, 8);
    }
    return -1;
}

// the workspace (workspace.hpp): per item one slot of partial sums and one of partial maxima
static float* stat_layout(const StatPlan& p, int64_t count, Workspace& ws) {
    return ws.take<float>(static_cast<size_t>(count) * static_cast<size_t>(p.slot) * 2 * sizeof(float), 8);
}

}  // namespace oq

extern "C" {

using namespace oq;

size_t oq_abs_stats_many_half_workspace_bytes(const oq_abs_stats_item* items_host, int64_t count) {
    StatPlan p;
    if (items_host == nullptr || count < 1 || count > 65535 || stat_plan(items_host, count, &p) >= 0) {
        set_error("oq_abs_stats_many_half_workspace_bytes: bad table (count=%lld)", (long long)count);
        return 0;
    }
    Workspace ws;
    stat_layout(p, count, ws);
    return ws.total();
}

int32_t oq_abs_stats_cols_many_h16(const oq_abs_stats_item* items_host, const oq_abs_stats_item* items_device, int64_t count, int32_t xtype,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(sizeof(oq_abs_stats_item) == 48 && sizeof(StatItem) == sizeof(oq_abs_stats_item), "six 8-byte fields");
    // every check on the host copy, before any arithmetic on an extent and before any HIP call
    int32_t st = half_operand_ok("oq_abs_stats_cols_many_h16", "x", xtype, nullptr);   // the items' X: entry by entry below
    if (st != OQ_OK) return st;
    OQ_REQUIRE(items_host != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_abs_stats_cols_many_h16: null items_host");
    OQ_REQUIRE(count >= 1 && count <= 65535, OQ_ERR_INVALID_ARGUMENT, "oq_abs_stats_cols_many_h16: bad count=%lld (1 <= count <= 65535)",
               (long long)count);
    OQ_REQUIRE(items_device != nullptr || count == 1, OQ_ERR_INVALID_ARGUMENT,
               "oq_abs_stats_cols_many_h16: null items_device (it may be NULL only when count == 1)");
    OQ_REQUIRE(aligned_to(items_device, 8), OQ_ERR_INVALID_ARGUMENT, "oq_abs_stats_cols_many_h16: items_device must be 8-byte aligned");
    for (int64_t i = 0; i < count; ++i) {
        const oq_abs_stats_item& it = items_host[i];
        OQ_REQUIRE(it.X != nullptr && it.abs_sum != nullptr && it.absmax != nullptr, OQ_ERR_INVALID_ARGUMENT,
                   "oq_abs_stats_cols_many_h16: item %lld: null X / abs_sum / absmax", (long long)i);
        OQ_REQUIRE(aligned_to(it.X, 2) && aligned_to(it.abs_sum, 4) && aligned_to(it.absmax, 4),
                   OQ_ERR_INVALID_ARGUMENT, "oq_abs_stats_cols_many_h16: item %lld: X must be 2-byte aligned, abs_sum and absmax 4-byte aligned",
                   (long long)i);
        OQ_REQUIRE(matrix_ok(it.T, it.K, it.ldx), OQ_ERR_INVALID_ARGUMENT, "oq_abs_stats_cols_many_h16: item %lld: bad shape T=%lld K=%lld ldx=%lld",
                   (long long)i, (long long)it.T, (long long)it.K, (long long)it.ldx);
    }
    StatPlan p;
    stat_plan(items_host, count, &p);
    Workspace ws(workspace, workspace_bytes);
    float* const partial = stat_layout(p, count, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "oq_abs_stats_cols_many_h16: workspace of %zu bytes needed, %zu given", ws.total(), workspace_bytes);
    // narrower loads while the table is too small to fill the device with waves at 8 columns per lane (a single 5120 x 640
    // tensor is 80 waves of them); the per-column sums do not depend on it
    const int cap = p.lanes8 >= kStatFillLanes ? 8 : (2 * p.lanes8 >= kStatFillLanes ? 4 : 2);
    int64_t grid_x = 1;
    for (int64_t i = 0; i < count; ++i) {
        const oq_abs_stats_item& it = items_host[i];
        const int v = stat_width(it.X, it.K, it.ldx, cap);
        const int64_t blocks = ceil_div(it.K, static_cast<int64_t>(kStatBlock) * v) * stat_chunks(it.T);   // < 2^23 x 64
        if (blocks > grid_x) grid_x = blocks;
    }
    const StatItem* table = count == 1 ? nullptr : reinterpret_cast<const StatItem*>(items_device);
    StatItem one;
    one.X = static_cast<const uint16_t*>(items_host[0].X);
    one.T = items_host[0].T;
    one.K = items_host[0].K;
    one.ldx = items_host[0].ldx;
    one.abs_sum = items_host[0].abs_sum;
    one.absmax = items_host[0].absmax;
    hipStream_t s = as_stream(stream);
    const dim3 grid(static_cast<uint32_t>(grid_x), static_cast<uint32_t>(count));
    with_half_elem(xtype, [&](auto e) { hipLaunchKernelGGL(abs_stats_half_partial<decltype(e)>, grid, dim3(kStatBlock), 0, s, table, one, cap, p.slot, partial); });
    st = check_launch("abs_stats_half_partial");
    if (st != OQ_OK) return st;
    const dim3 fgrid(static_cast<uint32_t>(ceil_div(p.max_k, kStatBlock)), static_cast<uint32_t>(count));
    hipLaunchKernelGGL(abs_stats_half_fold, fgrid, dim3(kStatBlock), 0, s, table, one, p.slot, static_cast<const float*>(partial));
    return check_launch("abs_stats_half_fold");
}

}  // extern "C"
