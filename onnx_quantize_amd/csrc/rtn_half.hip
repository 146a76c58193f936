// RTN weight quantization of fp16 / bf16 matrices for gfx950: the 2-byte W[K, N] is read as it is, never cast to an fp32 copy.
// Both conversions to fp32 are exact, so every result is by definition that of the fp32 kernels (rtn.hip) on the upcast matrix:
// the same R1 / Q1 (oq::qparam_from_minmax) and the same K1 (the reciprocal fast path with its exact redo, or oq::quantize_one).
//
//   group strategy, K % g == 0, g <= 256        one fused launch, W read once
//     g = 16 / 32 / 64 / 128 / 256              rtn_half_wave: a wave holds 128 (256) rows x 64 columns as PACKED halves in registers
//     every other g                             rtn_half_column: a thread per (group, column); the second read of its rows hits the L2
//     a LIST of matrices of one shape           the same two kernels with blockIdx.y = entry of a device table of pointers
//                                               (rtn_half_wave_many / rtn_half_column_many, oq_rtn_quantize_ptrs_h16)
//   channel, tensor, g > 256                    two launches over W (half_range + a fold, half_quantize): reading 2-byte W twice
//                                               costs what the fp32 kernels pay to read it once; nothing waits for another workgroup
//   with the MSE range search (oq_rtn_mse_h16)  the checks here, the search in rtn_mse.hip (templates on the element type), then
//                                               half_quantize with the stored parameters (launch_half_quantize_kn)
#include "rtn_internal.hpp"

#include "half_elem.hpp"

namespace oq {

struct HalfArgs {
    const uint16_t* W;
    int64_t K, N, ldw;
    int64_t g, kgroups;
    uint8_t* q;       // null: parameters only
    float* scale;
    uint8_t* zp;
    QGrid grid;
    int32_t layout;
    int32_t vec;      // 16-byte loads of W: N % 8 == 0, ldw % 8 == 0, 16-byte aligned base (host: picks the VEC build)
    int32_t qvec;     // [K,N] bytes: 8-byte stores (N % 8 == 0, 8-byte aligned output)
    int32_t spg;      // wave kernel: lane sets per group, g / R
    int32_t gk;       // wave kernel: row tiles per band of the block order
    uint32_t ncol_tiles, nrow_tiles;
    int32_t tensor;   // two-launch route: one parameter pair for the matrix
    int64_t chunks;   // two-launch route: range chunks per group
    float* pmin;
    float* pmax;
};

// The four pointers of one matrix: the fields of HalfArgs for a single matrix, an entry of the device table for a list
// (the layout of oq_rtn_ptrs_h16).
struct HalfPtrs {
    const uint16_t* W;
    uint8_t* q;       // null: parameters only
    float* scale;
    uint8_t* zp;
};

// Signed levels are biased by 128 so that every level is a byte v_cvt_pk_u8_f32 can place: the low nibble of level + 128 is the
// two's-complement nibble already, the byte needs bit 7 flipped back.
__device__ __forceinline__ int32_t level_bias(const QGrid& g) { return g.qmin < 0 ? 128 : 0; }

// 16 (8-bit: 4 words) or 16 (4-bit: 2 words) rows of one column of the MatMulNBits blob from four words of level bytes, rows
// ascending (qrules/_common.py:72-87: k ascending, even k in the low nibble).
__device__ __forceinline__ uint32_t nibble_word(uint32_t a, uint32_t b) {   // bytes [a0 a1 a2 a3], [b0 b1 b2 b3] -> [a0|a1<<4, a2|a3<<4, b0|b1<<4, b2|b3<<4]
    a &= 0x0f0f0f0fu; b &= 0x0f0f0f0fu;
    const uint32_t pa = a | (a >> 4), pb = b | (b >> 4);   // bytes 0 and 2 hold the pairs
    return (pa & 0xffu) | ((pa >> 8) & 0xff00u) | ((pb & 0xffu) << 16) | ((pb << 8) & 0xff000000u);
}

// ------------------------------------------------------------------------------------ fused, wave-owns-rows
// One wave = 8 * R rows x 64 columns.  Eight lanes span a row piece of 128 bytes (16 bytes = 8 halves each), the eight lane sets `h`
// hold R consecutive rows each: a lane keeps R x 4 registers of packed halves.  A group is `spg` = g / R neighbouring lane sets
// (1, 2, 4 or 8), its column ranges fold lane-locally and then across those lane sets on DPP / permlane swaps: no LDS, no barrier.
// In the blob a lane's R rows of a column are R / 2 (4-bit) or R (8-bit) consecutive bytes and the lane sets of a group adjacent,
// so one store instruction writes chunks of g / 2 (g) bytes, as the fp32 wave kernel does.  Rows are whole lane sets (K % g == 0,
// g % R == 0); lanes past an edge load a clamped address and store nothing.  VEC = false is the same kernel with 2-byte loads into
// the same registers, for rows that are not 16-byte aligned.
// Block order: that of the fp32 blob kernels (rtn.hip, order 2): bands of `gk` row tiles, ids blocked [8 column tiles] x [gk row tiles]
// with the column tile in the low bits, so neighbouring k-groups of a column tile run on one XCD and their pieces of a line meet in
// its L2.  Speed only: every tile is visited once.
// Three waves per SIMD for the 16-row build with vector loads (the hot path): 164 registers for fp16; bf16 would take 172 and
// fall to two waves, capped at 168 it parks two registers in scratch (docs/LAB_NOTES_r07.md: measured 40.6 / 55.9 us on
// 4096 x 11008 as built; the choice comes from the occupancy arithmetic, not from an A/B).
//
// The tile work is one __device__ body that takes the matrix' pointers: rtn_half_wave passes those of HalfArgs, rtn_half_wave_many
// those of entry blockIdx.y of a table.  PACKED adds the [K, N/2] epilogue (OQ_LAYOUT_KN_PACKED4) the list entry point offers: a
// lane's eight neighbouring columns of a row are two words of level bytes, its four packed bytes one nibble_word.
template <typename E, int R, bool VEC, bool PACKED>
__device__ __forceinline__ void half_wave_tile(const HalfArgs& a, const HalfPtrs m) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 3, cl = lane & 7;

    uint32_t row_tile, col_tile;
    {
        const uint32_t band_ids = a.ncol_tiles * static_cast<uint32_t>(a.gk);
        const uint32_t b = blockIdx.x / band_ids;
        uint32_t r = blockIdx.x - b * band_ids;
        const uint32_t gk_eff = min(static_cast<uint32_t>(a.gk), a.nrow_tiles - b * a.gk);
        const uint32_t cc = r / (8u * gk_eff);
        r -= cc * 8u * gk_eff;
        const uint32_t w = min(8u, a.ncol_tiles - cc * 8u);
        row_tile = b * a.gk + r / w;
        col_tile = cc * 8u + r % w;
    }
    const int64_t strip0 = (static_cast<int64_t>(col_tile) * 4 + wave) * 64;
    if (strip0 >= a.N) return;   // wave-uniform; nothing below synchronises across waves
    const int64_t tile_row0 = static_cast<int64_t>(row_tile) * (8 * R);
    const int64_t row0 = tile_row0 + h * R;
    const bool rows_ok = row0 < a.K;
    const int64_t col0 = strip0 + cl * 8;
    const int64_t kg = row0 / a.g;
    const int hs = h & (a.spg - 1);   // lane set inside its group

    bool cv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cv[j] = rows_ok && col0 + j < a.N;

    uint32_t v[R][4];
    {
        const int64_t lrow = rows_ok ? row0 : tile_row0;
        if constexpr (VEC) {   // N % 8 == 0: a lane's eight columns are in or out together
            const int64_t lc = col0 < a.N ? col0 : a.N - 8;
            const uint16_t* p = m.W + lrow * a.ldw + lc;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const u32x4 u = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + r * a.ldw));
                v[r][0] = u[0]; v[r][1] = u[1]; v[r][2] = u[2]; v[r][3] = u[3];
            }
        } else {       // rows that are not 16-byte aligned: 2-byte loads into the same registers
            int64_t c[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = col0 + j < a.N ? col0 + j : a.N - 1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint16_t* p = m.W + (lrow + r) * a.ldw;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[r][j] = static_cast<uint32_t>(p[c[2 * j]]) | (static_cast<uint32_t>(p[c[2 * j + 1]]) << 16);
            }
        }
    }

    // ---- R1: per-column range of the group, NaN-propagating (a NaN weight poisons exactly its group)
    float mn[8], mx[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        E::two(v[0][j], mn[2 * j], mn[2 * j + 1]);
        mx[2 * j] = mn[2 * j];
        mx[2 * j + 1] = mn[2 * j + 1];
    }
#pragma unroll
    for (int r = 1; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float lo, hi;
            E::two(v[r][j], lo, hi);
            mn[2 * j] = nmin(mn[2 * j], lo); mx[2 * j] = nmax(mx[2 * j], lo);
            mn[2 * j + 1] = nmin(mn[2 * j + 1], hi); mx[2 * j + 1] = nmax(mx[2 * j + 1], hi);
        }
    // the tile stays PACKED: without this the compiler keeps the 8 * R unpacked fp32 values of the range pass for K1 (128 more registers)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(v[r][j]));
    if (a.spg >= 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { mn[j] = xor_min<8>(mn[j]); mx[j] = xor_max<8>(mx[j]); }
    }
    if (a.spg >= 4) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { mn[j] = xor_min<16>(mn[j]); mx[j] = xor_max<16>(mx[j]); }
    }
    if (a.spg >= 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { mn[j] = xor_min<32>(mn[j]); mx[j] = xor_max<32>(mx[j]); }
    }

    // ---- Q1 and the constants of K1's fast path; lane set hs of a group stores the parameters of its share of the columns
    const int32_t qmin = a.grid.qmin, qmax = a.grid.qmax;
    const int32_t bias = level_bias(a.grid);
    float sc[8], rinv[8], zpb[8], thr = 1.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const QParam p = qparam_from_minmax(mn[j], mx[j], a.grid);
        const ColQ c = make_colq(p, mn[j], mx[j], bias);
        sc[j] = c.scale; rinv[j] = c.rinv; zpb[j] = c.zpb;
        thr = nmin(thr, c.thr);
        if (cv[j] && (j & (a.spg - 1)) == hs) {   // rtn.py:98-109 result layout: entry n * K/g + kg
            m.scale[(col0 + j) * a.kgroups + kg] = p.scale;
            m.zp[(col0 + j) * a.kgroups + kg] = static_cast<uint8_t>(p.zp);
        }
    }
    if (m.q == nullptr) return;

    const float lo_b = static_cast<float>(qmin + bias), hi_b = static_cast<float>(qmax + bias);
    // level (biased, an exact small float) of row r, column slot j
    auto level = [&](int r, int j, bool exact, bool& unsafe) -> float {
        float lo, hi;
        E::two(v[r][j >> 1], lo, hi);
        const float x = (j & 1) ? hi : lo;
        if (exact) return static_cast<float>(quantize_one(x, sc[j], static_cast<int32_t>(zpb[j]) - bias, qmin, qmax) + bias);
        const float t = x * rinv[j];
        const float k = rintf(t);
        unsafe = unsafe || !(fabsf(t - k) < thr);
        return __builtin_amdgcn_fmed3f(k + zpb[j], lo_b, hi_b);
    };

    const bool packed = PACKED && a.layout == OQ_LAYOUT_KN_PACKED4;
    if (a.layout == OQ_LAYOUT_KN || packed) {
        const uint32_t flip = bias ? 0x80808080u : 0u;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t w[2];
            auto row_words = [&](bool exact) -> bool {
                bool unsafe = false;
#pragma unroll
                for (int wd = 0; wd < 2; ++wd) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_cvt_pk_u8_f32(level(r, wd * 4 + i, exact, unsafe), i, acc);
                    w[wd] = acc ^ flip;
                }
                return unsafe;
            };
            if (__builtin_amdgcn_ballot_w64(row_words(false)) != 0) row_words(true);   // wave-uniform, rare: the IEEE divide
            if constexpr (PACKED) {
                if (packed) {   // even N (host): a pair of columns is in or out together; qvec: N % 8 == 0 and 4-byte aligned rows
                    const uint32_t pw = nibble_word(w[0], w[1]);
                    uint8_t* o = m.q + (row0 + r) * (a.N >> 1) + (col0 >> 1);
                    if (a.qvec) {
                        if (cv[0]) __builtin_nontemporal_store(pw, reinterpret_cast<uint32_t*>(o));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (cv[2 * i]) o[i] = static_cast<uint8_t>(pw >> (8 * i));
                    }
                    continue;
                }
            }
            uint8_t* o = m.q + (row0 + r) * a.N + col0;
            if (a.qvec) {
                if (cv[0]) __builtin_nontemporal_store(u32x2{w[0], w[1]}, reinterpret_cast<u32x2*>(o));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (cv[j]) o[j] = static_cast<uint8_t>(w[j >> 2] >> (8 * (j & 3)));
            }
        }
        return;
    }

    // ---- MatMulNBits blob: column by column, the R rows of a lane are consecutive bytes
    const bool four = a.grid.bits == 4;
    const uint32_t flip = bias ? 0x80808080u : 0u;
    const int64_t blob = a.g * a.grid.bits / 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t lw[R / 4];   // level bytes, rows ascending
        auto col_words = [&](bool exact) -> bool {
            bool unsafe = false;
#pragma unroll
            for (int wd = 0; wd < R / 4; ++wd) {
                uint32_t acc = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_cvt_pk_u8_f32(level(wd * 4 + i, j, exact, unsafe), i, acc);
                lw[wd] = acc;
            }
            return unsafe;
        };
        if (__builtin_amdgcn_ballot_w64(col_words(false)) != 0) col_words(true);   // wave-uniform, rare: the IEEE divide
        if (!cv[j]) continue;
        uint8_t* o = m.q + ((col0 + j) * a.kgroups + kg) * blob;
        if (four) {
            o += hs * (R / 2);
            if constexpr (R == 16) {
                *reinterpret_cast<u32x2*>(o) = u32x2{nibble_word(lw[0], lw[1]), nibble_word(lw[2], lw[3])};
            } else {
                *reinterpret_cast<u32x4*>(o) = u32x4{nibble_word(lw[0], lw[1]), nibble_word(lw[2], lw[3]), nibble_word(lw[4], lw[5]), nibble_word(lw[6], lw[7])};
            }
        } else {
            o += hs * R;
#pragma unroll
            for (int wd = 0; wd < R / 4; wd += 4)
                *reinterpret_cast<u32x4*>(o + 4 * wd) = u32x4{lw[wd] ^ flip, lw[wd + 1] ^ flip, lw[wd + 2] ^ flip, lw[wd + 3] ^ flip};
        }
    }
}

template <typename E, int R, bool VEC>
__global__ __launch_bounds__(256, R == 16 && VEC ? 3 : 1) void rtn_half_wave(const HalfArgs a) {
    half_wave_tile<E, R, VEC, false>(a, HalfPtrs{a.W, a.q, a.scale, a.zp});
}

// A list of matrices of one shape: blockIdx.y is the entry (wave-uniform: its four pointers come by scalar loads), blockIdx.x the tile in the single
// matrix' order, so every matrix keeps its bands.  A null table is a list of one, whose pointers are in HalfArgs.
// oq_rtn_quantize_h16 does not launch this form for its one matrix: on 4096 x 11008 it is up to 11 % slower than rtn_half_wave
// (g = 256, [K, N] bytes; docs/LAB_NOTES_r17.md).
template <typename E, int R, bool VEC>
__global__ __launch_bounds__(256, R == 16 && VEC ? 3 : 1) void rtn_half_wave_many(const HalfArgs a, const HalfPtrs* __restrict__ table) {
    half_wave_tile<E, R, VEC, true>(a, table != nullptr ? table[blockIdx.y] : HalfPtrs{a.W, a.q, a.scale, a.zp});
}

// ------------------------------------------------------------------------------------ plain kernels (a thread per column)
// K1 with stored parameters on rows [r0, r1) of column `col`; the IEEE division (oq::quantize_one).  [K,N] bytes, or -- whole slabs
// of 16 rows of one group -- 8 / 16 bytes of the blob.
template <typename E>
__device__ __forceinline__ void quantize_rows(const HalfArgs& a, const HalfPtrs& m, int64_t col, int64_t r0, int64_t r1, int64_t kg, float scale, int32_t zp) {
    const int32_t qmin = a.grid.qmin, qmax = a.grid.qmax;
    const uint16_t* w = m.W + col;
    if (a.layout == OQ_LAYOUT_KN) {
        for (int64_t r = r0; r < r1; ++r) m.q[r * a.N + col] = static_cast<uint8_t>(quantize_one(E::one(w[r * a.ldw]), scale, zp, qmin, qmax));
        return;
    }
    // g % 16 == 0 (host): [r0, r1) is a whole number of 16-row slabs of group kg
    const int64_t blob = a.g * a.grid.bits / 8;
    uint8_t* o = m.q + (col * a.kgroups + kg) * blob;
    for (int64_t r = r0; r < r1; r += 16) {
        uint32_t lw[4];
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            uint32_t acc = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc |= (static_cast<uint32_t>(quantize_one(E::one(w[(r + wd * 4 + i) * a.ldw]), scale, zp, qmin, qmax)) & 0xffu) << (8 * i);
            lw[wd] = acc;
        }
        const int64_t in_group = r - kg * a.g;
        if (a.grid.bits == 4) *reinterpret_cast<u32x2*>(o + in_group / 2) = u32x2{nibble_word(lw[0], lw[1]), nibble_word(lw[2], lw[3])};
        else *reinterpret_cast<u32x4*>(o + in_group) = u32x4{lw[0], lw[1], lw[2], lw[3]};
    }
}

// Fused, any g <= 256 with K % g == 0: a thread per (group, column), neighbouring threads on neighbouring columns.
template <typename E>
__device__ __forceinline__ void half_column_groups(const HalfArgs& a, const HalfPtrs m) {
    const int64_t kg = blockIdx.x / a.ncol_tiles;
    const int64_t col = static_cast<int64_t>(blockIdx.x % a.ncol_tiles) * 256 + threadIdx.x;
    if (col >= a.N) return;
    const int64_t r0 = kg * a.g, r1 = r0 + a.g;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t r = r0; r < r1; ++r) {
        const float x = E::one(m.W[r * a.ldw + col]);
        mn = nmin(mn, x);
        mx = nmax(mx, x);
    }
    const QParam p = qparam_from_minmax(mn, mx, a.grid);
    m.scale[col * a.kgroups + kg] = p.scale;
    m.zp[col * a.kgroups + kg] = static_cast<uint8_t>(p.zp);
    if (m.q != nullptr) quantize_rows<E>(a, m, col, r0, r1, kg, p.scale, p.zp);
}
template <typename E>
__global__ __launch_bounds__(256) void rtn_half_column(const HalfArgs a) {
    half_column_groups<E>(a, HalfPtrs{a.W, a.q, a.scale, a.zp});
}
// ... of entry blockIdx.y of a table (null: a list of one, in HalfArgs), as rtn_half_wave_many
template <typename E>
__global__ __launch_bounds__(256) void rtn_half_column_many(const HalfArgs a, const HalfPtrs* __restrict__ table) {
    half_column_groups<E>(a, table != nullptr ? table[blockIdx.y] : HalfPtrs{a.W, a.q, a.scale, a.zp});
}

// Two-launch route, launch 1: ranges of chunks of up to 64 rows of a group, [kgroups * chunks, N].
constexpr int64_t kHalfChunk = 64;
template <typename E>
__global__ __launch_bounds__(256) void half_range(const HalfArgs a) {
    const int64_t chunk = blockIdx.x / a.ncol_tiles;
    const int64_t col = static_cast<int64_t>(blockIdx.x % a.ncol_tiles) * 256 + threadIdx.x;
    if (col >= a.N) return;
    const int64_t kg = chunk / a.chunks, c = chunk - kg * a.chunks;
    const int64_t r0 = kg * a.g + c * kHalfChunk, r1 = min(r0 + kHalfChunk, kg * a.g + a.g);
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t r = r0; r < r1; ++r) {
        const float x = E::one(a.W[r * a.ldw + col]);
        mn = nmin(mn, x);
        mx = nmax(mx, x);
    }
    a.pmin[chunk * a.N + col] = mn;
    a.pmax[chunk * a.N + col] = mx;
}

// The fold of the chunk ranges into parameters: a thread per (group, column) ...
__global__ __launch_bounds__(256) void half_fold_columns(const HalfArgs a) {
    const int64_t kg = blockIdx.x / a.ncol_tiles;
    const int64_t col = static_cast<int64_t>(blockIdx.x % a.ncol_tiles) * 256 + threadIdx.x;
    if (col >= a.N) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t c = 0; c < a.chunks; ++c) {
        mn = nmin(mn, a.pmin[(kg * a.chunks + c) * a.N + col]);
        mx = nmax(mx, a.pmax[(kg * a.chunks + c) * a.N + col]);
    }
    const QParam p = qparam_from_minmax(mn, mx, a.grid);
    a.scale[col * a.kgroups + kg] = p.scale;
    a.zp[col * a.kgroups + kg] = static_cast<uint8_t>(p.zp);
}
// ... or one block for the one pair of a tensor
__global__ __launch_bounds__(1024) void half_fold_tensor(const HalfArgs a) {
    __shared__ float s_mn[16], s_mx[16];
    const int64_t count = a.chunks * a.N;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < count; i += 1024) {
        mn = nmin(mn, a.pmin[i]);
        mx = nmax(mx, a.pmax[i]);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { mn = nmin(mn, s_mn[w]); mx = nmax(mx, s_mx[w]); }
        const QParam p = qparam_from_minmax(mn, mx, a.grid);
        a.scale[0] = p.scale;
        a.zp[0] = static_cast<uint8_t>(p.zp);
    }
}

// Two-launch route, launch 2: a thread per (slab of 16 rows of a group, column).
template <typename E>
__global__ __launch_bounds__(256) void half_quantize(const HalfArgs a) {
    const int64_t slab = blockIdx.x / a.ncol_tiles;
    const int64_t col = static_cast<int64_t>(blockIdx.x % a.ncol_tiles) * 256 + threadIdx.x;
    if (col >= a.N) return;
    const int64_t spg = (a.g + 15) / 16;   // slabs per group; the last one of a group may be short ([K,N] layout only)
    const int64_t kg = slab / spg, s = slab - kg * spg;
    const int64_t r0 = kg * a.g + s * 16, r1 = min(r0 + 16, kg * a.g + a.g);
    const int64_t pi = a.tensor ? 0 : col * a.kgroups + kg;
    const int32_t zp = a.grid.qmin < 0 ? static_cast<int32_t>(static_cast<int8_t>(a.zp[pi])) : static_cast<int32_t>(a.zp[pi]);
    quantize_rows<E>(a, HalfPtrs{a.W, a.q, a.scale, a.zp}, col, r0, r1, kg, a.scale[pi], zp);
}

// ------------------------------------------------------------------------------------ host
static bool half_fused(int32_t strategy, int64_t g) { return strategy == OQ_GROUP && g <= 256; }
static bool half_wave_group(int64_t g) { return g == 16 || g == 32 || g == 64 || g == 128 || g == 256; }   // rtn_half_wave has a build for it

static size_t half_workspace(int32_t strategy, int64_t K, int64_t N, int64_t g) {
    if (half_fused(strategy, g)) return 0;
    return static_cast<size_t>(2 * (K / g) * ceil_div(g, kHalfChunk) * N) * sizeof(float);
}

// The fused route (half_fused): one launch of `batch` matrices of one shape.  LIST: entry b at table[b] (device memory; null:
// batch == 1, the pointers are in `a`), the entry as grid y, the table kernels; otherwise the one matrix of `a` and the
// single-matrix kernels.  The wave / column choice, the tile shape and the block order are one for both.
template <typename E, bool LIST>
static int32_t half_launch_fused(HalfArgs& a, const HalfPtrs* table, int64_t batch, hipStream_t s) {
    const int64_t g = a.g;
    const dim3 block(256);
    if (half_wave_group(g)) {
        const int rows = g == 256 ? 32 : 16;
        a.spg = static_cast<int32_t>(g / rows);
        a.nrow_tiles = static_cast<uint32_t>(ceil_div(a.K, 8 * rows));
        a.gk = 4;
        const dim3 grid(a.ncol_tiles * a.nrow_tiles, static_cast<uint32_t>(batch));
        if constexpr (LIST) {
            if (rows == 16) {
                if (a.vec) hipLaunchKernelGGL((rtn_half_wave_many<E, 16, true>), grid, block, 0, s, a, table);
                else hipLaunchKernelGGL((rtn_half_wave_many<E, 16, false>), grid, block, 0, s, a, table);
            } else {
                if (a.vec) hipLaunchKernelGGL((rtn_half_wave_many<E, 32, true>), grid, block, 0, s, a, table);
                else hipLaunchKernelGGL((rtn_half_wave_many<E, 32, false>), grid, block, 0, s, a, table);
            }
            return check_launch("rtn_half_wave_many");
        } else {
            if (rows == 16) {
                if (a.vec) hipLaunchKernelGGL((rtn_half_wave<E, 16, true>), grid, block, 0, s, a);
                else hipLaunchKernelGGL((rtn_half_wave<E, 16, false>), grid, block, 0, s, a);
            } else {
                if (a.vec) hipLaunchKernelGGL((rtn_half_wave<E, 32, true>), grid, block, 0, s, a);
                else hipLaunchKernelGGL((rtn_half_wave<E, 32, false>), grid, block, 0, s, a);
            }
            return check_launch("rtn_half_wave");
        }
    }
    const dim3 grid(a.ncol_tiles * static_cast<uint32_t>(a.kgroups), static_cast<uint32_t>(batch));
    if constexpr (LIST) {
        hipLaunchKernelGGL(rtn_half_column_many<E>, grid, block, 0, s, a, table);
        return check_launch("rtn_half_column_many");
    } else {
        hipLaunchKernelGGL(rtn_half_column<E>, grid, block, 0, s, a);
        return check_launch("rtn_half_column");
    }
}

// K1 with the stored parameters of `a`: launch 2 of the two-launch route, and (launch_half_quantize_kn) the final pass of the MSE search.
template <typename E>
static int32_t half_launch_quantize(const HalfArgs& a, hipStream_t s) {
    const int64_t slabs = a.kgroups * ceil_div(a.g, 16);
    hipLaunchKernelGGL(half_quantize<E>, dim3(a.ncol_tiles * static_cast<uint32_t>(slabs)), dim3(256), 0, s, a);
    return check_launch("half_quantize");
}

int32_t launch_half_quantize_kn(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int64_t g, int64_t kgroups, float* scale,
                                uint8_t* zp, uint8_t* q, const QGrid& grid, bool tensor, hipStream_t s) {
    HalfArgs a{};
    a.W = static_cast<const uint16_t*>(W);
    a.K = K; a.N = N; a.ldw = ldw; a.g = g; a.kgroups = kgroups;
    a.q = q; a.scale = scale; a.zp = zp;
    a.grid = grid;
    a.layout = OQ_LAYOUT_KN;
    a.ncol_tiles = static_cast<uint32_t>(ceil_div(N, 256));
    a.tensor = tensor ? 1 : 0;
    return with_half_elem(wtype, [&](auto e) { return half_launch_quantize<decltype(e)>(a, s); });
}

// The two-launch route of the one matrix of `a`: channel, tensor, groups taller than 256 rows.
template <typename E>
static int32_t half_launch(HalfArgs& a, hipStream_t s) {
    const int64_t g = a.g;
    a.chunks = ceil_div(g, kHalfChunk);
    hipLaunchKernelGGL(half_range<E>, dim3(a.ncol_tiles * static_cast<uint32_t>(a.kgroups * a.chunks)), dim3(256), 0, s, a);
    int32_t st = check_launch("half_range");
    if (st != OQ_OK) return st;
    if (a.tensor) {
        a.chunks *= a.kgroups;
        hipLaunchKernelGGL(half_fold_tensor, dim3(1), dim3(1024), 0, s, a);
    } else {
        hipLaunchKernelGGL(half_fold_columns, dim3(a.ncol_tiles * static_cast<uint32_t>(a.kgroups)), dim3(256), 0, s, a);
    }
    st = check_launch("half_fold");
    if (st != OQ_OK || a.q == nullptr) return st;
    return half_launch_quantize<E>(a, s);
}

// What oq_rtn_quantize_h16, oq_rtn_mse_h16 and oq_rtn_quantize_ptrs_h16 (`fn`) check alike, before any arithmetic on an extent and
// before any HIP call; fills the shape, the grid, the group and the layout of `a`.  `W`: the one matrix, null for a table of them.
static int32_t half_checks(const char* fn, const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype, int32_t strategy, int64_t group_size,
                           int32_t symmetric, int32_t reduce_range, float clip_ratio, int32_t layout, HalfArgs* a) {
    int32_t st = half_operand_ok(fn, "W", wtype, W);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(K > 0 && N > 0 && ldw >= N, OQ_ERR_INVALID_ARGUMENT, "%s: bad shape K=%lld N=%lld ldw=%lld", fn, (long long)K, (long long)N,
               (long long)ldw);
    OQ_REQUIRE(matrix_ok(K, N, ldw), OQ_ERR_UNSUPPORTED, "%s: matrix too large (K=%lld N=%lld ldw=%lld)", fn, (long long)K, (long long)N,
               (long long)ldw);
    OQ_REQUIRE(clip_ratio > 0.0f && clip_ratio <= 1.0f, OQ_ERR_INVALID_ARGUMENT, "clip_ratio must be in (0.0, 1.0], got %g", clip_ratio);
    OQ_REQUIRE(layout == OQ_LAYOUT_KN || layout == OQ_LAYOUT_NBITS || layout == OQ_LAYOUT_KN_PACKED4, OQ_ERR_INVALID_ARGUMENT, "%s: bad layout %d", fn,
               layout);
    st = make_grid(qtype, symmetric, reduce_range, clip_ratio, &a->grid);
    if (st != OQ_OK) return st;
    int64_t g;
    st = resolve_group(strategy, K, group_size, &g);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(K % g == 0, OQ_ERR_UNSUPPORTED,
               "%s: group_size %lld does not divide K=%lld (groups that straddle columns have no half-precision kernel)", fn, (long long)g,
               (long long)K);
    a->K = K; a->N = N; a->ldw = ldw; a->g = g; a->kgroups = K / g;
    a->layout = layout;
    a->ncol_tiles = static_cast<uint32_t>(ceil_div(N, 256));
    // the largest grid of any route: a block per (16-row slab or group, 256 columns)
    OQ_REQUIRE(static_cast<int64_t>(a->ncol_tiles) * a->kgroups * ceil_div(g, 16) <= kMaxExtent, OQ_ERR_UNSUPPORTED,
               "%s: matrix too large for one launch (K=%lld N=%lld)", fn, (long long)K, (long long)N);
    return OQ_OK;
}

}  // namespace oq

extern "C" {

int32_t oq_half_extension_version(void) { return OQ_HALF_EXTENSION_VERSION; }

size_t oq_rtn_half_workspace_bytes(int64_t K, int64_t N, int32_t strategy, int64_t group_size) {
    if (!oq::matrix_ok(K, N, N)) {
        oq::set_error("oq_rtn_half_workspace_bytes: bad shape K=%lld N=%lld", (long long)K, (long long)N);
        return 0;
    }
    int64_t g;
    if (oq::resolve_group(strategy, K, group_size, &g) != OQ_OK) return 0;
    if (strategy == OQ_GROUP && K % g != 0) {
        oq::set_error("oq_rtn_half_workspace_bytes: groups that straddle columns (K %% group_size != 0) have no half-precision kernel");
        return 0;
    }
    return oq::half_workspace(strategy, K, N, g);
}

int32_t oq_rtn_quantize_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype, int32_t strategy,
                            int64_t group_size, int32_t symmetric, int32_t reduce_range, float clip_ratio, void* q_out,
                            float* scale_out, void* zp_out, int32_t layout, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace oq;
    // every check before any arithmetic on an extent and before any HIP call
    OQ_REQUIRE(W != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_h16: null W");
    OQ_REQUIRE(scale_out != nullptr && zp_out != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_h16: null scale_out / zp_out");
    OQ_REQUIRE(aligned_to(scale_out, 4), OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_h16: scale_out must be 4-byte aligned");
    HalfArgs a{};
    const int32_t st = half_checks("oq_rtn_quantize_h16", W, wtype, K, N, ldw, qtype, strategy, group_size, symmetric, reduce_range, clip_ratio, layout, &a);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(layout != OQ_LAYOUT_KN_PACKED4, OQ_ERR_UNSUPPORTED,
               "oq_rtn_quantize_h16: layout KN_PACKED4 is not produced here; quantize to KN and pack with oq_pack_nibbles");
    const int64_t g = a.g;
    if (layout == OQ_LAYOUT_NBITS) {
        OQ_REQUIRE(strategy == OQ_GROUP && q_out != nullptr, OQ_ERR_UNSUPPORTED, "oq_rtn_quantize_h16: NBITS layout needs the group strategy and q_out");
        OQ_REQUIRE(g % 16 == 0 && aligned_to(q_out, 16), OQ_ERR_UNSUPPORTED,
                   "oq_rtn_quantize_h16: NBITS layout needs group_size %% 16 == 0 and a 16-byte aligned q_out");
    }
    const size_t need = half_workspace(strategy, K, N, g);
    OQ_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need && aligned_to(workspace, 4)), OQ_ERR_WORKSPACE,
               "oq_rtn_quantize_h16: workspace of %zu bytes (4-byte aligned) needed, %zu given", need, workspace ? workspace_bytes : static_cast<size_t>(0));

    a.W = static_cast<const uint16_t*>(W);
    a.q = static_cast<uint8_t*>(q_out); a.scale = scale_out; a.zp = static_cast<uint8_t*>(zp_out);
    a.vec = (N % 8 == 0 && ldw % 8 == 0 && aligned_to(W, 16)) ? 1 : 0;
    a.qvec = (N % 8 == 0 && aligned_to(q_out, 8)) ? 1 : 0;
    a.tensor = strategy == OQ_TENSOR ? 1 : 0;
    if (need != 0) {
        a.pmin = static_cast<float*>(workspace);
        a.pmax = a.pmin + need / (2 * sizeof(float));
    }
    const hipStream_t s = as_stream(stream);
    return with_half_elem(wtype, [&](auto e) {
        return half_fused(strategy, g) ? half_launch_fused<decltype(e), false>(a, nullptr, 1, s) : half_launch<decltype(e)>(a, s);
    });
}

size_t oq_rtn_mse_half_workspace_bytes(int64_t K, int64_t N, int32_t strategy, int64_t group_size) {
    if (!oq::matrix_ok(K, N, N)) {
        oq::set_error("oq_rtn_mse_half_workspace_bytes: bad shape K=%lld N=%lld", (long long)K, (long long)N);
        return 0;
    }
    int64_t g;
    if (oq::resolve_group(strategy, K, group_size, &g) != OQ_OK) return 0;
    if (strategy == OQ_GROUP && K % g != 0) {
        oq::set_error("oq_rtn_mse_half_workspace_bytes: groups that straddle columns (K %% group_size != 0) have no MSE search");
        return 0;
    }
    return oq::rtn_mse_workspace(K, N, strategy, g);
}

int32_t oq_rtn_mse_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype, int32_t strategy, int64_t group_size,
                       int32_t symmetric, int32_t reduce_range, float clip_ratio, void* q_out, float* scale_out, void* zp_out, int32_t layout,
                       void* workspace, size_t workspace_bytes, void* stream) {
    using namespace oq;
    static const char fn[] = "oq_rtn_mse_h16";
    // every check before any arithmetic on an extent and before any HIP call
    OQ_REQUIRE(W != nullptr, OQ_ERR_INVALID_ARGUMENT, "%s: null W", fn);
    OQ_REQUIRE(scale_out != nullptr && zp_out != nullptr, OQ_ERR_INVALID_ARGUMENT, "%s: null scale_out / zp_out", fn);
    OQ_REQUIRE(aligned_to(scale_out, 4), OQ_ERR_INVALID_ARGUMENT, "%s: scale_out must be 4-byte aligned", fn);
    HalfArgs a{};
    const int32_t st = half_checks(fn, W, wtype, K, N, ldw, qtype, strategy, group_size, symmetric, reduce_range, clip_ratio, layout, &a);
    if (st != OQ_OK) return st;
    OQ_REQUIRE(layout == OQ_LAYOUT_KN, OQ_ERR_UNSUPPORTED, "%s: layout %s with mse is not supported (the MSE search writes [K, N] bytes)", fn,
               layout == OQ_LAYOUT_NBITS ? "NBITS" : "KN_PACKED4");
    // the search's grid: a block per (256 columns, group) with the group as y; the resolve pass: a thread per (column, group)
    OQ_REQUIRE(strategy == OQ_TENSOR || (a.kgroups <= 65535 && ceil_div(N * a.kgroups, 256) <= kMaxExtent), OQ_ERR_UNSUPPORTED,
               "%s: more than 65535 groups per column or too many groups for one launch (K=%lld N=%lld group_size %lld)", fn, (long long)K,
               (long long)N, (long long)a.g);
    const size_t need = rtn_mse_workspace(K, N, strategy, a.g);
    OQ_REQUIRE(workspace != nullptr && workspace_bytes >= need && aligned_to(workspace, 4), OQ_ERR_WORKSPACE,
               "%s: workspace of %zu bytes (4-byte aligned) needed, %zu given", fn, need, workspace ? workspace_bytes : static_cast<size_t>(0));
    // clip_ratio is validated and then not applied: the MSE range replaces the clipped one (rtn_mse_impl)
    return rtn_mse_half_impl(W, wtype, K, N, ldw, a.grid, strategy, a.g, q_out, scale_out, zp_out, workspace, workspace_bytes, as_stream(stream));
}

int32_t oq_rtn_quantize_ptrs_h16(const oq_rtn_ptrs_h16* table_host, const oq_rtn_ptrs_h16* table_device, int64_t count, int32_t wtype,
                                 int64_t K, int64_t N, int64_t ldw, int32_t qtype, int64_t group_size, int32_t symmetric,
                                 int32_t reduce_range, float clip_ratio, int32_t layout, void* stream) {
    using namespace oq;
    static_assert(sizeof(HalfPtrs) == sizeof(oq_rtn_ptrs_h16) && sizeof(oq_rtn_ptrs_h16) == sizeof(oq_rtn_ptrs), "device view of oq_rtn_ptrs_h16");
    // every check on the host copy, before any arithmetic on an extent and before any HIP call
    OQ_REQUIRE(table_host != nullptr, OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_ptrs_h16: null table_host");
    OQ_REQUIRE(count >= 1 && count <= 65535, OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_ptrs_h16: count %lld outside 1 .. 65535", (long long)count);
    OQ_REQUIRE(table_device != nullptr || count == 1, OQ_ERR_INVALID_ARGUMENT,
               "oq_rtn_quantize_ptrs_h16: null table_device with count %lld (it may be null for count 1 only)", (long long)count);
    HalfArgs a{};
    int32_t st = half_checks("oq_rtn_quantize_ptrs_h16", nullptr, wtype, K, N, ldw, qtype, OQ_GROUP, group_size, symmetric, reduce_range, clip_ratio, layout, &a);
    if (st != OQ_OK) return st;
    const int64_t g = a.g;
    OQ_REQUIRE(half_fused(OQ_GROUP, g), OQ_ERR_UNSUPPORTED,
               "oq_rtn_quantize_ptrs_h16: group_size %lld is taller than the fused kernels hold (256 rows); call oq_rtn_quantize_h16 per matrix",
               (long long)g);
    if (layout == OQ_LAYOUT_NBITS)
        OQ_REQUIRE(g % 16 == 0, OQ_ERR_UNSUPPORTED, "oq_rtn_quantize_ptrs_h16: NBITS layout needs group_size %% 16 == 0, got %lld", (long long)g);
    if (layout == OQ_LAYOUT_KN_PACKED4) {
        OQ_REQUIRE(a.grid.bits == 4, OQ_ERR_UNSUPPORTED, "oq_rtn_quantize_ptrs_h16: KN_PACKED4 layout needs a 4-bit type");
        OQ_REQUIRE(N % 2 == 0, OQ_ERR_UNSUPPORTED, "oq_rtn_quantize_ptrs_h16: KN_PACKED4 layout needs an even number of columns, got N=%lld", (long long)N);
        OQ_REQUIRE(half_wave_group(g), OQ_ERR_UNSUPPORTED,
                   "oq_rtn_quantize_ptrs_h16: KN_PACKED4 layout needs a group_size of 16, 32, 64, 128 or 256 (the wave kernel), got %lld", (long long)g);
    }
    // the load and store widths are chosen for the call: every entry has to meet what they promise, or the call runs the narrow build
    bool vec = N % 8 == 0 && ldw % 8 == 0, qvec = N % 8 == 0;
    const uintptr_t q_store = layout == OQ_LAYOUT_KN_PACKED4 ? 4 : 8;
    for (int64_t i = 0; i < count; ++i) {
        const oq_rtn_ptrs_h16& p = table_host[i];
        OQ_REQUIRE(p.W && p.q_out && p.scale_out && p.zp_out, OQ_ERR_INVALID_ARGUMENT, "oq_rtn_quantize_ptrs_h16: null pointer in entry %lld", (long long)i);
        OQ_REQUIRE(aligned_to(p.W, 2) && aligned_to(p.scale_out, 4), OQ_ERR_INVALID_ARGUMENT,
                   "oq_rtn_quantize_ptrs_h16: entry %lld: W must be 2-byte aligned and scale_out 4-byte aligned", (long long)i);
        OQ_REQUIRE(layout != OQ_LAYOUT_NBITS || aligned_to(p.q_out, 16), OQ_ERR_UNSUPPORTED,
                   "oq_rtn_quantize_ptrs_h16: entry %lld: NBITS layout needs a 16-byte aligned q_out", (long long)i);
        vec = vec && aligned_to(p.W, 16);
        qvec = qvec && aligned_to(p.q_out, q_store);
    }
    a.vec = vec ? 1 : 0;
    a.qvec = qvec ? 1 : 0;

    // How many matrices share a launch (blockIdx.y = entry): the rule of the fp32 entry point, oq::matrices_per_launch.
    const int64_t per_launch = matrices_per_launch(K, N, count);
    const hipStream_t s = as_stream(stream);
    for (int64_t i = 0; i < count; i += per_launch) {
        const int64_t batch = count - i < per_launch ? count - i : per_launch;
        const HalfPtrs* table = table_device != nullptr ? reinterpret_cast<const HalfPtrs*>(table_device) + i : nullptr;
        const oq_rtn_ptrs_h16& p = table_host[i];   // read by the kernel only where there is no device table (count == 1)
        a.W = static_cast<const uint16_t*>(p.W);
        a.q = static_cast<uint8_t*>(p.q_out); a.scale = p.scale_out; a.zp = static_cast<uint8_t*>(p.zp_out);
        st = with_half_elem(wtype, [&](auto e) { return half_launch_fused<decltype(e), true>(a, table, batch, s); });
        if (st != OQ_OK) return st;
    }
    return OQ_OK;
}

}  // extern "C"
