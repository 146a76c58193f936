// M1: the MSE range search of utils.py:140-239 for gfx950.
//
// For every row of the reference's preprocessed layout (a k-group of one output channel, a whole output
// channel, or the whole tensor) the reference shrinks the (min, max) range by p = 1 - i/100, i = 0..19,
// fake-quantizes the row with the parameters of the shrunk range and keeps the range with the smallest
// sum |q - x|^2.4.  Its stop rule is GLOBAL: it counts the iterations in which no row at all improved and
// stops at the fifth (the counter is never reset, utils.py:232-237).
//
// Here every row records a 20-bit mask of the iterations in which it would improve (rows are independent
// until the stop), the masks are OR-ed into one device word, and a resolve kernel derives the stop
// iteration from that word and picks, per row, the last improving iteration not after it.  The search is
// ALU-bound (an IEEE divide and |d|^2.4 per element and candidate, 20 candidates); W is re-read from
// L2 / Infinity Cache per candidate instead of being tiled (g > 128), or held in registers (g = 32 / 64 / 128, and 256 of a 2-byte matrix, mse_rows_reg_kernel: the division
// there is the proven-equal reciprocal product of the RTN kernels with an exact redo inside the tie band).  The power runs on the hardware log / exp units (the library
// powf was 3/4 of the kernel: 4.6 -> 1.2 ms on the 4096 x 11008 matrix).
//
// Numerics: per-element arithmetic follows the reference (divide, rint, clamp, (q - zp) * s, subtract, abs,
// |.|^2.4), but NumPy's pow kernel and its pairwise summation order cannot be reproduced bit for bit,
// so two candidates whose errors differ in the last bits can swap.  tests/test_mse_gpu.py judges every row on its own
// (tests/mse_verdict.py): a band tau = summation order + the two 1-ulp instructions + NumPy's own distance from a float64
// evaluation, about 1e-5 to 4e-5 and never above 1e-4, is derived per case from the reference's arithmetic; a row whose best
// candidate leads by more than 2 tau must equal the reference bit for bit, and the others (under 1 % of the rows) must stay
// within 2 tau of the best.
//
// Tiny magnitudes: v_log_f32 / v_exp_f32 neither take nor return subnormal numbers, NumPy's power does.  With weights around
// 1e-15 most terms |d|^2.4 are subnormal while the row sums are still normal, and the reference goes on searching down to
// 1e-18.  Rows whose unshrunk scale is below 2^kMseShiftBelow therefore take a second path: the exponent of the hardware
// exp2 is moved up by 12 j (j = -exponent / 5, so 2.4 * 5 j is an exact integer), which keeps it in the normal range, and
// v_ldexp_f32 moves the result back with ONE rounding to the subnormal grid, which is what a correctly rounded power does.
// The choice is wave-uniform: a wave without such a row runs the instructions it ran before.  An ordinary row that shares a
// wave with a tiny one takes the second path with a shift of 0 (fma(2.4, L, +0) is the rounded product, ldexp by 0 the
// identity, and the plain division is what the reciprocal path is proved equal to), so its bits do not change either;
// test_mse_tiny_and_ordinary_columns_in_one_wave holds it to that.
//
// Element types: W is fp32, fp16 or bf16 (oq_rtn_mse_h16, oq_hip_half.h).  The kernels that read W are templates on the element
// (ElemF32 / ElemF16 / ElemBF16 of half_elem.hpp); the 2-byte types are read as they are and converted exactly at the load, and
// everything behind the load -- the arithmetic per element and candidate, the order of every sum, the grid-stride mapping and the
// block count of the tensor route, the tie-band redo, the shifted power, the masks and the resolve -- is one source for all three.
// So the search on a half matrix gives the bytes of the fp32 search on the upcast matrix (tests/test_mse_half_gpu.py), and the
// fp32 instantiations are the kernels this file had before it was a template.  Groups of 256 of a 2-byte matrix have a register
// tile too (packed, see mse_rows_reg_kernel); the final pass of a half matrix is rtn_half.hip's stored-parameter pass.
#include "rtn_internal.hpp"

#include "half_elem.hpp"

namespace oq {

constexpr int kMseSteps = 20;      // int(maxshrink * grid) = int(0.20 * 100.0), utils.py:197
constexpr int kMsePatience = 5;    // utils.py:150
constexpr float kMseNorm = 2.4f;   // utils.py:152
constexpr int kMseChunk = 16;      // elements per tie-band check of the register kernel
constexpr int kMseShiftBelow = -32;  // rows whose unshrunk scale is below 2^-32 compute |d|^2.4 through mse_pow_shift

// candidate i: p = 1 - i / 100.0 (Python float), applied to fp32 ranges as a weak scalar -> fp32 product
__device__ __forceinline__ float shrink_factor(int i) { return static_cast<float>(1.0 - static_cast<double>(i) / 100.0); }

__device__ __forceinline__ float fake_quant_error(float x, const QParam& p, const QGrid& g) {
    const int32_t q = quantize_one(x, p.scale, p.zp, g.qmin, g.qmax);
    const float d = dequantize_one(q, p.scale, p.zp) - x;
    // |d|^2.4 = 2^(2.4 log2 |d|) on the hardware log / exp units (~2e-6 relative; the library powf costs several times
    // the rest of the candidate, and NumPy's own float32 pow is not reproduced bit for bit either way, see above)
    return __builtin_amdgcn_exp2f(kMseNorm * __builtin_amdgcn_logf(fabsf(d)));
}

// 0 for ordinary rows; otherwise the (negative, multiple of 12) power of two that brings 2^(2.4 log2 |d| - shift) back.
// A scale of 1 (the tiny-range guard), inf and NaN have exponents >= 0 and give 0.
__device__ __forceinline__ int mse_pow_shift(float lo0, float hi0, const QGrid& g) {
    const QParam p0 = qparam_from_range(lo0, hi0, g);
    const int e = static_cast<int>((__float_as_uint(p0.scale) >> 23) & 0xffu) - 127;
    return e < kMseShiftBelow ? 12 * (e / 5) : 0;
}

__device__ __forceinline__ float fake_quant_error_shifted(float x, const QParam& p, const QGrid& g, int shift) {
    const int32_t q = quantize_one(x, p.scale, p.zp, g.qmin, g.qmax);
    const float d = dequantize_one(q, p.scale, p.zp) - x;
    const float up = __builtin_amdgcn_exp2f(fmaf(kMseNorm, __builtin_amdgcn_logf(fabsf(d)), static_cast<float>(-shift)));
    return ldexpf(up, shift);   // shift == 0: the bits of fake_quant_error
}

struct MseRow {
    float lo0, hi0;   // utils.py:188 range with clip_ratio = 1.0, zero included
    uint32_t mask;    // bit i: iteration i improves this row (no early stop assumed)
};

// channel / group: one thread per (column, k-group); lanes walk neighbouring columns -> coalesced rows
template <typename E>
__global__ __launch_bounds__(256) void mse_rows_kernel(const typename E::raw* W, int64_t K, int64_t N, int64_t ldw, int64_t g,
                                                       int64_t kgroups, QGrid grid, MseRow* rows, uint32_t* any_mask) {
    const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t kg = blockIdx.y;
    const bool live = n < N;
    const int64_t nc = live ? n : N - 1;
    const typename E::raw* col = W + kg * g * ldw + nc;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t r = 0; r < g; ++r) {
        const float x = E::one(col[r * ldw]);
        mn = nmin(mn, x);
        mx = nmax(mx, x);
    }
    const float lo0 = nmin(mn, 0.0f), hi0 = nmax(mx, 0.0f);
    float best = FLT_MAX;   // np.finfo(float32).max, utils.py:190
    uint32_t mask = 0;
    const int shift = mse_pow_shift(lo0, hi0, grid);
    const bool shifted = __builtin_amdgcn_ballot_w64(shift != 0) != 0;
    for (int i = 0; i < kMseSteps; ++i) {
        const float p = shrink_factor(i);
        const QParam qp = qparam_from_range(p * lo0, p * hi0, grid);
        float err = 0.f;
        if (shifted) {
            for (int64_t r = 0; r < g; ++r) err += fake_quant_error_shifted(E::one(col[r * ldw]), qp, grid, shift);
        } else {
            for (int64_t r = 0; r < g; ++r) err += fake_quant_error(E::one(col[r * ldw]), qp, grid);
        }
        if (err < best) {  // utils.py:225
            best = err;
            mask |= 1u << i;
        }
    }
    if (live) {
        MseRow o;
        o.lo0 = lo0; o.hi0 = hi0; o.mask = mask;
        rows[n * kgroups + kg] = o;
    }
    // block-wide OR, one atomic per wave
    uint32_t m = live ? mask : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, 64);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(any_mask, m);
}

// The same search with the group's G values held in REGISTERS across the 20 candidates: W is read once
// (G strided 4-byte loads per thread, coalesced across the lanes of a row) instead of 21 times from L2 / Infinity Cache,
// and the candidate loop is pure ALU.  Same per-element arithmetic and the same summation order (r = 0 .. G-1 into one fp32
// accumulator) as mse_rows_kernel: bit-identical masks.  G <= 128 keeps the tile within 256 VGPRs (two waves per SIMD: an
// ALU-bound loop with G independent chains per candidate needs no more).
//
// Element types: fp32 as it is; fp16 / bf16 converted exactly at the load for G <= 128 (the tile is the fp32 one from there on).
// G = 256 exists for the 2-byte types only and keeps the tile PACKED, elements 2 i and 2 i + 1 of the group in one register (128
// registers; as fp32 the tile alone would be the whole budget of two waves per SIMD): a chunk's 16 elements are unpacked where a
// candidate uses them.  Same chunks, same order of the sum: the masks mse_rows_kernel gives at g = 256.  Every lane loads one
// element a row, so rows that are only 2-byte aligned need no path of their own.
template <typename E, int G>
__global__ __launch_bounds__(256, 2) void mse_rows_reg_kernel(const typename E::raw* W, int64_t N, int64_t ldw, int64_t kgroups, QGrid grid,
                                                             MseRow* rows, uint32_t* any_mask) {
    typedef typename E::raw raw;
    constexpr bool kPacked = G > 128;
    static_assert(G % kMseChunk == 0 && G <= 256 && (!kPacked || sizeof(raw) == 2), "register tile");
    const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t kg = blockIdx.y;
    const bool live = n < N;
    const int64_t nc = live ? n : N - 1;
    // wave-uniform row base + one 32-bit lane offset for all G loads (no 64-bit per-lane address per row)
    const char* base = reinterpret_cast<const char*>(W + kg * G * ldw);
    const uint32_t lane_off = static_cast<uint32_t>(nc) * static_cast<uint32_t>(sizeof(raw));
    const int64_t row_bytes = ldw * static_cast<int64_t>(sizeof(raw));
    float x[kPacked ? 1 : G];
    uint32_t xp[kPacked ? G / 2 : 1];
    (void)x; (void)xp;
    float mn, mx;
    if constexpr (kPacked) {
        // 16 loads in flight, then their 8 packed registers, pinned HERE (the device of hqq_rounds_reg_kernel): left alone all 256
        // loads are issued first, each into a register of its own, and the tile spills on the way.  The range is folded batch by
        // batch from the pinned registers, r = 0 .. G-1 as below.
        mn = mx = 0.f;
#pragma unroll
        for (int tb = 0; tb < G; tb += 16) {
#pragma unroll
            for (int u = 0; u < 16; u += 2)
                xp[(tb + u) / 2] = static_cast<uint32_t>(*reinterpret_cast<const raw*>(base + (tb + u) * row_bytes + lane_off)) |
                                   (static_cast<uint32_t>(*reinterpret_cast<const raw*>(base + (tb + u + 1) * row_bytes + lane_off)) << 16);
            asm volatile("" : "+v"(xp[tb / 2]), "+v"(xp[tb / 2 + 1]), "+v"(xp[tb / 2 + 2]), "+v"(xp[tb / 2 + 3]), "+v"(xp[tb / 2 + 4]),
                              "+v"(xp[tb / 2 + 5]), "+v"(xp[tb / 2 + 6]), "+v"(xp[tb / 2 + 7]));
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float v = E::one(static_cast<raw>(xp[(tb + u) / 2] >> (16 * (u & 1))));
                mn = tb + u == 0 ? v : nmin(mn, v);
                mx = tb + u == 0 ? v : nmax(mx, v);
            }
            asm volatile("" : "+v"(mn), "+v"(mx));   // the batch's range exists before the next batch's loads land
        }
    } else {
#pragma unroll
        for (int r = 0; r < G; ++r) x[r] = E::one(*reinterpret_cast<const raw*>(base + r * row_bytes + lane_off));
        mn = x[0]; mx = x[0];
#pragma unroll
        for (int r = 1; r < G; ++r) {
            mn = nmin(mn, x[r]);
            mx = nmax(mx, x[r]);
        }
    }
    const float lo0 = nmin(mn, 0.0f), hi0 = nmax(mx, 0.0f);
    float best = FLT_MAX;   // np.finfo(float32).max, utils.py:190
    uint32_t mask = 0;
    const bool shifted = __builtin_amdgcn_ballot_w64(mse_pow_shift(lo0, hi0, grid) != 0) != 0;
#pragma unroll 1
    for (int i = 0; i < kMseSteps; ++i) {
        const float p = shrink_factor(i);
        const QParam qp = qparam_from_range(p * lo0, p * hi0, grid);
        // the division-free level of oq_common.hpp (proved equal to the reference's integer away from rounding ties), in
        // chunks of 16 elements: a chunk in which any lane of the wave sits inside the tie band (~1 % of the chunks) is
        // redone with the true division by the whole wave.  Same values, same summation order as the plain loop.
        const ColQ c = make_colq(qp, mn, mx, 0);
        const float lo_f = static_cast<float>(grid.qmin), hi_f = static_cast<float>(grid.qmax);
        float err = 0.f;
        // (unroll(full): `#pragma unroll` leaves the 16 chunks of G = 256 rolled, and a rolled loop indexes the tile in scratch)
#pragma clang loop unroll(full)
        for (int r0 = 0; r0 < G; r0 += kMseChunk) {
            float e[kMseChunk];
            float off = 0.f;   // max |t - rint(t)| of the chunk (t is finite whenever c.thr > 0, make_colq)
            // one chunk at a time: its reciprocal is opaque until the previous chunk's sum exists (left alone, the compiler
            // runs several chunks' temporaries at once and spills the tile at G = 128)
            float rinv = c.rinv;
            asm volatile("" : "+v"(rinv), "+v"(err));
            // the chunk's values: the tile's own registers, or unpacked HERE from the chunk's 8 packed ones (opaque per candidate:
            // the unpacked values do not change from candidate to candidate, and kept they are the fp32 tile)
            float xu[kPacked ? kMseChunk : 1];
            (void)xu;
            if constexpr (kPacked) {
                asm volatile("" : "+v"(xp[r0 / 2]), "+v"(xp[r0 / 2 + 1]), "+v"(xp[r0 / 2 + 2]), "+v"(xp[r0 / 2 + 3]), "+v"(xp[r0 / 2 + 4]),
                                  "+v"(xp[r0 / 2 + 5]), "+v"(xp[r0 / 2 + 6]), "+v"(xp[r0 / 2 + 7]));
#pragma unroll
                for (int r = 0; r < kMseChunk; ++r) xu[r] = E::one(static_cast<raw>(xp[(r0 + r) / 2] >> (16 * (r & 1))));
            }
            const float* xc = kPacked ? xu : x + r0;
#pragma unroll
            for (int r = 0; r < kMseChunk; ++r) {
                const float t = xc[r] * rinv;
                const float k = rintf(t);
                off = fmaxf(off, fabsf(t - k));
                const float lvl = __builtin_amdgcn_fmed3f(k + c.zpb, lo_f, hi_f);
                const float d = (lvl - c.zpb) * c.scale - xc[r];
                e[r] = __builtin_amdgcn_exp2f(kMseNorm * __builtin_amdgcn_logf(fabsf(d)));
            }
            if (shifted) {   // tiny magnitudes (wave-uniform, see the header): the plain division and the shifted power
                const int shift = mse_pow_shift(lo0, hi0, grid);
#pragma unroll
                for (int r = 0; r < kMseChunk; ++r) e[r] = fake_quant_error_shifted(xc[r], qp, grid, shift);
            } else if (__builtin_amdgcn_ballot_w64(!(off < c.thr)) != 0) {
#pragma unroll
                for (int r = 0; r < kMseChunk; ++r) e[r] = fake_quant_error(xc[r], qp, grid);
            }
#pragma unroll
            for (int r = 0; r < kMseChunk; ++r) err += e[r];
        }
        if (err < best) {  // utils.py:225
            best = err;
            mask |= 1u << i;
        }
    }
    if (live) {
        MseRow o;
        o.lo0 = lo0; o.hi0 = hi0; o.mask = mask;
        rows[n * kgroups + kg] = o;
    }
    uint32_t m = live ? mask : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, 64);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(any_mask, m);
}

// tensor: per-block partial sums of all 20 candidate errors
template <typename E>
__global__ __launch_bounds__(256) void mse_tensor_partial(const typename E::raw* W, int64_t K, int64_t N, int64_t ldw, const float* range,
                                                          QGrid grid, float* partial /* [blocks][20] */) {
    __shared__ float s_sum[4][kMseSteps];
    const float lo0 = nmin(range[0], 0.0f), hi0 = nmax(range[1], 0.0f);
    QParam qp[kMseSteps];
#pragma unroll
    for (int i = 0; i < kMseSteps; ++i) qp[i] = qparam_from_range(shrink_factor(i) * lo0, shrink_factor(i) * hi0, grid);
    float acc[kMseSteps];
#pragma unroll
    for (int i = 0; i < kMseSteps; ++i) acc[i] = 0.f;
    const int64_t total = K * N;
    const int shift = mse_pow_shift(lo0, hi0, grid);   // one range: uniform over the launch
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
         t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t k = t / N, n = t - k * N;
        const float x = E::one(W[k * ldw + n]);
        if (shift != 0) {
#pragma unroll
            for (int i = 0; i < kMseSteps; ++i) acc[i] += fake_quant_error_shifted(x, qp[i], grid, shift);
        } else {
#pragma unroll
            for (int i = 0; i < kMseSteps; ++i) acc[i] += fake_quant_error(x, qp[i], grid);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kMseSteps; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) s_sum[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kMseSteps)
        partial[static_cast<int64_t>(blockIdx.x) * kMseSteps + threadIdx.x] =
            (s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x]) + (s_sum[2][threadIdx.x] + s_sum[3][threadIdx.x]);
}

__global__ void mse_tensor_mask(const float* partial, int nblocks, const float* range, MseRow* row, uint32_t* any_mask) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float best = FLT_MAX;
    uint32_t mask = 0;
    for (int i = 0; i < kMseSteps; ++i) {
        float err = 0.f;
        for (int b = 0; b < nblocks; ++b) err += partial[b * kMseSteps + i];
        if (err < best) { best = err; mask |= 1u << i; }
    }
    row->lo0 = nmin(range[0], 0.0f);
    row->hi0 = nmax(range[1], 0.0f);
    row->mask = mask;
    *any_mask = mask;
}

// raw (min, max) of the whole tensor -> range[2] (single block; the tensor strategy is the plumbing case)
template <typename E>
__global__ __launch_bounds__(1024) void tensor_minmax_kernel(const typename E::raw* W, int64_t K, int64_t N, int64_t ldw, float* range) {
    __shared__ float s_mn[16], s_mx[16];
    float mn = INFINITY, mx = -INFINITY;
    const int64_t total = K * N;
    for (int64_t t = threadIdx.x; t < total; t += blockDim.x) {
        const int64_t k = t / N, n = t - k * N;
        const float x = E::one(W[k * ldw + n]);
        mn = nmin(mn, x);
        mx = nmax(mx, x);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { mn = nmin(mn, s_mn[w]); mx = nmax(mx, s_mx[w]); }
        range[0] = mn;
        range[1] = mx;
    }
}

// Stop iteration from the global mask (utils.py:232-237), then per row: last improving iteration not after it.
__device__ __forceinline__ int stop_iteration(uint32_t any_mask) {
    int stale = 0;
    for (int i = 0; i < kMseSteps; ++i) {
        if (!((any_mask >> i) & 1u)) ++stale;
        if (stale >= kMsePatience) return i;   // iteration i is the last one executed
    }
    return kMseSteps - 1;
}

__global__ void mse_resolve_kernel(const MseRow* rows, int64_t count, const uint32_t* any_mask, QGrid grid, float* scale,
                                   uint8_t* zp) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= count) return;
    const int last = stop_iteration(*any_mask);
    const uint32_t m = rows[r].mask & (last >= 31 ? 0xffffffffu : ((2u << last) - 1u));
    // best_min/max start as the unshrunk range (utils.py:191-192): that is also candidate 0
    const int idx = m ? 31 - __builtin_clz(m) : 0;
    const float p = shrink_factor(idx);
    const QParam qp = qparam_from_range(p * rows[r].lo0, p * rows[r].hi0, grid);  // utils.py:345-347 (clip ratio not applied)
    scale[r] = qp.scale;
    zp[r] = static_cast<uint8_t>(qp.zp);
}

// The search's workspace, measured and carved by this one function (workspace.hpp).
struct MseWs {
    uint32_t* any_mask;   // the stop word
    float* range;         // tensor strategy: raw (min, max) of the matrix
    MseRow* rowbuf;       // [rows]
    float* partial;       // tensor strategy: [blocks, kMseSteps] partial errors
};
constexpr int kMseTensorBlocks = 1024;

static MseWs mse_layout(int64_t K, int64_t N, int32_t strategy, int64_t g, Workspace& ws) {
    const int64_t rows = strategy == OQ_TENSOR ? 1 : N * (K / g);
    MseWs w;
    char* const head = ws.take(256);      // a unit of its own for the two small ones; the sizes are those of include/oq_hip_half.h, to the byte
    w.any_mask = reinterpret_cast<uint32_t*>(head);
    w.range = head ? reinterpret_cast<float*>(head + 16) : nullptr;
    w.rowbuf = ws.take<MseRow>(static_cast<size_t>(rows) * sizeof(MseRow), alignof(MseRow));
    w.partial = ws.take<float>(static_cast<size_t>(kMseTensorBlocks) * kMseSteps * sizeof(float), 4);
    return w;
}

size_t rtn_mse_workspace(int64_t K, int64_t N, int32_t strategy, int64_t g) {
    Workspace ws;
    mse_layout(K, N, strategy, g, ws);
    return ws.total();
}

// The search itself, from the cleared stop word to the resolved (scale, zp) of every row: one implementation for the three
// element types.  `grid` is the search's own (clip_ratio 1).
template <typename E>
static int32_t mse_search(const typename E::raw* W, int64_t K, int64_t N, int64_t ldw, const QGrid& grid, int32_t strategy, int64_t g,
                          float* scale_out, void* zp_out, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int64_t kgroups = strategy == OQ_TENSOR ? 1 : K / g;
    const int64_t rows = strategy == OQ_TENSOR ? 1 : N * kgroups;
    Workspace ws(workspace, workspace_bytes);
    const MseWs w = mse_layout(K, N, strategy, g, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "rtn(mse): workspace of %zu bytes needed, %zu given", ws.total(), workspace ? workspace_bytes : size_t{0});
    uint32_t* any_mask = w.any_mask;
    float* range = w.range;
    MseRow* rowbuf = w.rowbuf;
    float* partial = w.partial;
    if (hipMemsetAsync(any_mask, 0, 4, s) != hipSuccess) return fail(OQ_ERR_LAUNCH, "rtn(mse): memset failed");
    int32_t st;
    if (strategy == OQ_TENSOR) {
        const int nblocks = kMseTensorBlocks;
        hipLaunchKernelGGL(tensor_minmax_kernel<E>, dim3(1), dim3(1024), 0, s, W, K, N, ldw, range);
        hipLaunchKernelGGL(mse_tensor_partial<E>, dim3(nblocks), dim3(256), 0, s, W, K, N, ldw, range, grid, partial);
        hipLaunchKernelGGL(mse_tensor_mask, dim3(1), dim3(64), 0, s, partial, nblocks, range, rowbuf, any_mask);
        st = check_launch("mse_tensor");
    } else {
        const dim3 gd(static_cast<uint32_t>(ceil_div(N, 256)), static_cast<uint32_t>(kgroups));
        constexpr bool half = sizeof(typename E::raw) == 2;   // group 256: the packed tile, which exists for the 2-byte types only
        if (g == 128) hipLaunchKernelGGL((mse_rows_reg_kernel<E, 128>), gd, dim3(256), 0, s, W, N, ldw, kgroups, grid, rowbuf, any_mask);
        else if (g == 64) hipLaunchKernelGGL((mse_rows_reg_kernel<E, 64>), gd, dim3(256), 0, s, W, N, ldw, kgroups, grid, rowbuf, any_mask);
        else if (g == 32) hipLaunchKernelGGL((mse_rows_reg_kernel<E, 32>), gd, dim3(256), 0, s, W, N, ldw, kgroups, grid, rowbuf, any_mask);
        else if (half && g == 256) {
            if constexpr (half) hipLaunchKernelGGL((mse_rows_reg_kernel<E, 256>), gd, dim3(256), 0, s, W, N, ldw, kgroups, grid, rowbuf, any_mask);
        } else hipLaunchKernelGGL(mse_rows_kernel<E>, gd, dim3(256), 0, s, W, K, N, ldw, g, kgroups, grid, rowbuf, any_mask);
        st = check_launch("mse_rows_kernel");
    }
    if (st != OQ_OK) return st;
    hipLaunchKernelGGL(mse_resolve_kernel, dim3(static_cast<uint32_t>(ceil_div(rows, 256))), dim3(256), 0, s, rowbuf, rows, any_mask, grid,
                       scale_out, static_cast<uint8_t*>(zp_out));
    return check_launch("mse_resolve_kernel");
}

int32_t rtn_mse_impl(const float* W, int64_t K, int64_t N, int64_t ldw, const QGrid& grid_in, int32_t strategy, int64_t g,
                     void* q_out, float* scale_out, void* zp_out, int32_t zp_signed, void* workspace, size_t workspace_bytes,
                     hipStream_t s, bool emit_q) {
    QGrid grid = grid_in;
    grid.clip_ratio = 1.0f;  // utils.py:188 and :334-344: the MSE range replaces the clipped one
    const int64_t kgroups = strategy == OQ_TENSOR ? 1 : K / g;
    const int32_t st = mse_search<ElemF32>(W, K, N, ldw, grid, strategy, g, scale_out, zp_out, workspace, workspace_bytes, s);
    if (st != OQ_OK || !emit_q) return st;
    return launch_quantize_kn(W, K, N, ldw, g, kgroups, scale_out, static_cast<const uint8_t*>(zp_out), static_cast<uint8_t*>(q_out),
                              grid, zp_signed, strategy == OQ_TENSOR, s, OQ_LAYOUT_KN);
}

// oq_rtn_mse_h16 (rtn_half.hip makes every check): the same search on the 2-byte matrix, then the stored-parameter pass of the
// half kernels (IEEE division: the integers launch_quantize_kn gives on the upcast matrix).
int32_t rtn_mse_half_impl(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, const QGrid& grid_in, int32_t strategy, int64_t g,
                          void* q_out, float* scale_out, void* zp_out, void* workspace, size_t workspace_bytes, hipStream_t s) {
    QGrid grid = grid_in;
    grid.clip_ratio = 1.0f;  // as above
    const uint16_t* w = static_cast<const uint16_t*>(W);
    const int32_t st = with_half_elem(wtype, [&](auto e) { return mse_search<decltype(e)>(w, K, N, ldw, grid, strategy, g, scale_out, zp_out, workspace, workspace_bytes, s); });
    if (st != OQ_OK || q_out == nullptr) return st;
    return launch_half_quantize_kn(W, wtype, K, N, ldw, g, strategy == OQ_TENSOR ? 1 : K / g, scale_out, static_cast<uint8_t*>(zp_out),
                                   static_cast<uint8_t*>(q_out), grid, strategy == OQ_TENSOR, s);
}

}  // namespace oq
