// One call of a `quant`-domain QDQ function with quantized activations run from a 4-bit weight as the file stores it
// (include/oq_hip_qdq_function_packed4.h): an ONNX INT4 / UINT4 initializer [K, N] with an even N, i.e. a [K, N / 2]
// byte matrix, value [k, 2 j] in the low nibble of byte [k, j].  fp32 X in, fp32 Y out, the product on v_mfma_i32_16x16x64_i8.
//
//       q_x[m, k] = the static quantizer, or DynamicQuantizeLinear's with the parameters of X          qdq_function_parts.hpp
//       B[k, n]   = W[k, n] - zp_w[n]                       an int8 in [-15, 15], formed while W is staged
//       S[m, n]   = sum_k (q_x[m, k] - zp_x) * B[k, n]      exact, int32
//       Y         = the epilogue of qdq_function.hip (finish_qdq) on S, with B signed and without a zero point
//
// Everything around the product -- the min / max pass, the parameter kernel, the quantizing prologue (launched without row sums:
// their multiplier zb' is zero), the split-K reduce, the finish of a dynamic output, the plan and the workspace -- is
// qdq_function_parts.hpp, the text qdq_function.hip runs.  This file's own: the tile GEMM body below, which shares the A staging,
// the MFMA loop and the epilogue's calls with ql_gemm_body (qlinear_tile.hpp) line for line but stages B from nibbles, and the
// column sums of the centred B.  A body of its own rather than a third arm of ql_gemm_body: the image has other rows, the
// fragments other addresses, the staging other registers, and the kernels of five files are held to that body's text.
//
//   staging   a 64-k x 128-column step is 64 rows of 64 bytes: 4 dwords for each of the 256 threads (the byte route loads 8).  Thread
//             t owns dword cb = t & 15 of a row -- the columns 8 cb ... 8 cb + 7 -- at the 4 consecutive k = 4 kq ... 4 kq + 3,
//             kq = t >> 4 (qdq_matmul_packed4.hip's assignment): a quarter wave lies on the 64 consecutive bytes of one row.  A loaded
//             dword d, flipped nibble by nibble for a signed W (d ^ 0x88888888: q + 8 as an unsigned nibble), splits into
//             e = d & 0x0F0F0F0F, the four even columns as bytes, and o = (d >> 4) & 0x0F0F0F0F, the four odd ones.  The zero
//             points of the thread's eight columns are loaded once per call as bytes, flipped likewise, and sorted into ze / zo, the
//             even and the odd columns' four.  ((e | 0x80808080) - ze) ^ 0x80808080 subtracts byte by byte: 128 + w - z lies in
//             113 ... 143, so no byte borrows, and flipping bit 7 back leaves the two's complement of w - z in [-15, 15].  The two
//             4 x 4 byte blocks (4 columns x 4 k) are then transposed with the v_perm_b32 network of ql_gemm_body, which leaves the
//             4 consecutive k of one column in a dword: 8 writes of 4 bytes per thread and step, at byte 4 kq of the column's row.
//   image     [n][k] bytes, rows of kRow = 80 bytes (64 of k and 16 of padding, as in qlinear_gemm.hip), from which a lane reads its
//             fragment of v_mfma_i32_16x16x64_i8 as 16 bytes: lane & 15 the column, lane >> 4 the k quarter.  LDS has 64 banks of 4
//             bytes; a row is 20 banks, 5 bank quads.
//             With row = column, the 16 lanes that write one k run of the columns 8 cb + c start in bank 20 (8 cb + c) + kq =
//             160 cb + const, and 160 cb mod 64 takes two values: an 8-way conflict.  Here column 8 cb + c lies in image row
//             18 c + cb (kColPlane = 18; 7 * 18 + 16 = 142 rows for 128 columns: 14 padding rows of 80 bytes), so the rows of
//             neighbouring lanes are neighbours.
//             writes: one write instruction has c fixed.  A wave is cb = 0 ... 15 at kq = kq0 ... kq0 + 3, kq0 a multiple of 4; its
//             dwords lie in bank 20 (18 c + cb) + kq = const + 20 cb + (kq - kq0) mod 64.  20 cb mod 64 = 4 (5 cb mod 16) takes the
//             16 multiples of 4 once each (5 is a unit mod 16), kq - kq0 fills the 4 banks between: 64 lanes, 64 different banks.
//             reads: the 16 columns of fragment nt of column half wn are 64 wn + 16 nt + l, l = lane & 15: cb = 8 wn + 2 nt +
//             (l >> 3), c = l & 7, so the row is 18 (l & 7) + (l >> 3) + 8 wn + 2 nt.  Their 16 bytes start in bank quad
//             5 row + (lane >> 4) mod 16; 5 is a unit mod 16 and 18 c + h = 2 c + h mod 16, c = 0 ... 7, h = 0, 1, takes all 16
//             residues: 16 lanes, 16 different bank quads, as the reads of qlinear_gemm.hip's image.
//   guards    those of qdq_matmul_packed4.hip: rows >= M and k >= K of A are zeros in LDS.  No byte outside [K, N / 2] of W and no
//             zero point outside its tensor is read: a thread whose k run past K or whose columns run past N reads the last row /
//             byte / column again, which meets those zeros of A or lands in outputs that are never stored.  No load is guarded on
//             its own.  Rows of W that are not 4-byte aligned, and the last columns of an N that is no multiple of 8, are read byte
//             by byte.
//   sums      sum_k (W - zp)[n] over a slice of K = (sum of the unsigned nibbles) - rows * zp_u[n].  A block takes 128 columns of one
//             slice as 16 dwords x 16 phases of k; the even and the odd nibbles of a dword are added as packed bytes for 17 rows
//             (17 * 15 = 255) and then widened.  The layout is the [kColSlices][colsum_stride] col_terms reads.
// Built with the packed fp32 instructions switched off (_build.py), like qdq_matmul_packed4.hip.
#include "qdq_function_parts.hpp"

#include "../../include/oq_hip_qdq_function_packed4.h"

namespace oq {
namespace {

constexpr int64_t kMaxK = 561433;     // 255 * 15 * K <= 2^31 - 1: no int32 sum can wrap
constexpr int kColPlane = 18;         // rows of the B image between columns 8 cb + c and 8 cb + c + 1
constexpr int kImageRows = 7 * kColPlane + kBN / 8;

struct Packed4FnArgs : QdqArgs {      // B / ldb: W and its leading dimension in bytes; b_vec: rows of W are 4-byte aligned;
    const uint8_t* w_zp;              // b_zp is NULL (the epilogue's B has no zero point); W's: one byte per tensor / column, NULL: 0
    int32_t w_per_column;
    uint32_t nibble_flip;             // 0x88888888 for a signed W
};

constexpr int p4_gemm_lds_bytes(int mt) { return (32 * mt + kImageRows) * kRow; }

// r[i]: bytes of columns j = 0 ... 3 at k + i  ->  c[j]: bytes of k ... k + 3 of column j (the selectors of ql_gemm_body)
__device__ __forceinline__ void transpose4x4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&c)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
    const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u), c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u), c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// four unsigned nibbles as bytes minus four zero points as bytes, byte by byte: each byte the two's complement of w - z
__device__ __forceinline__ uint32_t sub_bytes(uint32_t w4, uint32_t z4) { return ((w4 | 0x80808080u) - z4) ^ 0x80808080u; }

// `lds`: p4_gemm_lds_bytes(MT) bytes, 16-byte aligned, declared by the kernel
template <int MT>
__device__ __forceinline__ void p4_gemm_body(const Packed4FnArgs& p, unsigned char* const lds) {
    constexpr int BM = 32 * MT;
    constexpr int NT = 4;
    constexpr int A_CHUNKS = (BM * 4 + kThreads - 1) / kThreads;      // 16-byte chunks of the A tile per thread
    unsigned char* const lds_b = lds + BM * kRow;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t m0 = (tile % p.tiles_m) * BM, n0 = (tile / p.tiles_m) * kBN;      // below 2^31 + a tile
    const uint32_t k_begin = blockIdx.y * p.steps_per_split * kBK;                                 // below K + 64 splits
    const uint32_t k_end = min(p.K, k_begin + p.steps_per_split * kBK);

    u32x4 a_regs[A_CHUNKS];
    const uint8_t* a_row[A_CHUNKS];      // the row of chunk i; NULL: a row >= M, or no chunk (the 32-row tile has 128)
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) {
        const int id = tid + i * kThreads;
        const uint32_t m = m0 + (id >> 2);
        a_row[i] = (id < BM * 4 && m < p.M) ? p.A + static_cast<int64_t>(m) * p.lda : nullptr;
    }

    // B: this thread's dword cb of the step's rows 4 kq ... 4 kq + 3, i.e. the columns pn ... pn + 7
    const int cb = tid & 15, kq = tid >> 4;
    const uint32_t pn = n0 + 8 * cb;
    const bool b_dword = p.b_vec != 0 && pn + 8 <= p.N;
    const int b_last = static_cast<int>(min(3u, ((p.N - min(pn, p.N - 2u)) >> 1) - 1u));      // N is even: the last byte of the thread that exists
    uint32_t b_regs[4] = {0u, 0u, 0u, 0u};
    uint32_t ze = 0u, zo = 0u;           // the flipped zero points of the even / odd four of the eight columns
    if (p.w_zp != nullptr && pn < p.N) {
        uint32_t raw[2] = {0u, 0u};
        const uint8_t* z = p.w_zp + (p.w_per_column ? pn : 0u);      // walks the eight columns and stays on the last one that exists
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            raw[c >> 2] |= static_cast<uint32_t>(*z) << (8 * (c & 3));
            if (p.w_per_column && pn + c + 1 < p.N) ++z;
        }
        raw[0] = (raw[0] ^ p.nibble_flip) & 0x0F0F0F0Fu, raw[1] = (raw[1] ^ p.nibble_flip) & 0x0F0F0F0Fu;
        ze = __builtin_amdgcn_perm(raw[1], raw[0], 0x06040200u), zo = __builtin_amdgcn_perm(raw[1], raw[0], 0x07050301u);
    } else {
        ze = zo = p.nibble_flip & 0x0F0F0F0Fu;      // a missing zero point is the flip of 0
    }

    auto load_step = [&](uint32_t k) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            a_regs[i] = u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
            if (a_row[i]) a_regs[i] = load_k16(a_row[i], k + (tid & 3) * 16, p.K, p.a_vec != 0, p.a_flip);
        }
        // Nothing below is guarded load by load: a row past K repeats row K - 1, a byte past N / 2 byte N / 2 - 1.  All meet zeros of
        // A or belong to outputs that are never stored.
        const uint32_t kk = k + 4 * kq;
#pragma unroll
        for (int i = 0; i < 4; ++i) b_regs[i] = 0u;
        if (kk < k_end && pn < p.N) {
            const uint8_t* src = p.B + static_cast<int64_t>(kk) * p.ldb + (pn >> 1);
            if (b_dword) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b_regs[i] = *reinterpret_cast<const uint32_t*>(src);
                    if (kk + i + 1 < p.K) src += p.ldb;
                }
            } else {
                const int o1 = min(1, b_last), o2 = min(2, b_last);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b_regs[i] = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[o1]) << 8) | (static_cast<uint32_t>(src[o2]) << 16) |
                                (static_cast<uint32_t>(src[b_last]) << 24);
                    if (kk + i + 1 < p.K) src += p.ldb;
                }
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * kThreads;
            if (id < BM * 4) *reinterpret_cast<u32x4*>(lds + (id >> 2) * kRow + (id & 3) * 16) = a_regs[i] ^ u32x4{p.a_flip, p.a_flip, p.a_flip, p.a_flip};
        }
        uint32_t e[4], o[4], even[4], odd[4];      // even[j]: k ... k + 3 of column pn + 2 j;  odd[j]: of column pn + 2 j + 1
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = b_regs[i] ^ p.nibble_flip;
            e[i] = sub_bytes(r & 0x0F0F0F0Fu, ze), o[i] = sub_bytes((r >> 4) & 0x0F0F0F0Fu, zo);
        }
        transpose4x4(e[0], e[1], e[2], e[3], even);
        transpose4x4(o[0], o[1], o[2], o[3], odd);
        unsigned char* const dst = lds_b + cb * kRow + 4 * kq;
#pragma unroll
        for (int c = 0; c < 8; ++c) *reinterpret_cast<uint32_t*>(dst + kColPlane * c * kRow) = c & 1 ? odd[c >> 1] : even[c >> 1];
    };

    i32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = i32x4{0, 0, 0, 0};

    const unsigned char* const a_frag = lds + (wm * 16 * MT + (lane & 15)) * kRow + (lane >> 4) * 16;
    const unsigned char* const b_frag = lds_b + (kColPlane * (lane & 7) + ((lane & 15) >> 3) + 8 * wn) * kRow + (lane >> 4) * 16;      // + 2 nt rows

    if (k_begin < k_end) load_step(k_begin);
    for (uint32_t k = k_begin; k < k_end; k += kBK) {
        store_step();
        __syncthreads();
        if (k + kBK < k_end) load_step(k + kBK);
        i32x4 b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = *reinterpret_cast<const i32x4*>(b_frag + 2 * nt * kRow);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const i32x4 a = *reinterpret_cast<const i32x4*>(a_frag + mt * 16 * kRow);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 MFMAs: column = lane & 15, row = 4 (lane >> 4) + r
    const uint32_t col = n0 + wn * 64 + (lane & 15);
    MinMax mm;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const uint32_t n = col + 16 * nt;
        if (n >= p.N) continue;
        ColTerms c{};
        float bias = 0.0f;
        if (!p.slab) c = col_terms(p, n), bias = qdq_bias(p, n);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m = m0 + wm * 16 * MT + mt * 16 + 4 * (lane >> 4) + r;
                if (m < p.M) {
                    const uint32_t S = static_cast<uint32_t>(acc[mt][nt][r]);
                    if (p.slab) p.slab[(static_cast<int64_t>(blockIdx.y) * p.M + m) * p.N + n] = S;
                    else finish_qdq(p, m, n, S, c, bias, mm);
                }
            }
    }
    // the k loop's last barrier is behind every read of the tiles: LDS is free
    if (!p.slab && p.out_mode == kQdqDynamic) block_minmax_store(mm, reinterpret_cast<float*>(lds), p.pairs, blockIdx.x);
}

template <int MT>
__global__ __launch_bounds__(kThreads, 2) void qp_gemm_kernel(const Packed4FnArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[p4_gemm_lds_bytes(MT)];
    p4_gemm_body<MT>(p, lds);
}

// sums[y][n] = sum over slice y of K of (W[k, n] - zp[n]): grid (ceil(N / 128), kColSlices).  `NB`: N / 2, the bytes of a row.
__global__ __launch_bounds__(kThreads) void qp_sum_cols_kernel(const uint8_t* W, uint32_t K, uint32_t N, int64_t ldw, int32_t vec, uint32_t flip,
                                                               const uint8_t* zp, int32_t per_column, int32_t* sums, uint32_t stride) {
    __shared__ uint32_t part[16][kBN];
    const int cg = threadIdx.x & 15, ph = threadIdx.x >> 4;
    const uint32_t NB = N / 2u, byte0 = blockIdx.x * 64u + 4u * cg;
    const uint32_t per_slice = (K + gridDim.y - 1u) / gridDim.y, k_begin = min(K, blockIdx.y * per_slice), k_end = min(K, k_begin + per_slice);
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};      // s[2 b], s[2 b + 1]: the low and the high nibbles of byte b
    if (byte0 < NB) {
        uint32_t lo = 0u, hi = 0u;
        int rows = 0;
        auto widen = [&]() {
#pragma unroll
            for (int b = 0; b < 4; ++b) s[2 * b] += (lo >> (8 * b)) & 0xFFu, s[2 * b + 1] += (hi >> (8 * b)) & 0xFFu;
            lo = hi = 0u, rows = 0;
        };
        // past N / 2: zeros (load_n4) ^ flip, the sums of columns that are never stored
        for (uint32_t k = k_begin + ph; k < k_end; k += 16u) {
            const uint32_t w = load_n4(W + static_cast<int64_t>(k) * ldw + byte0, byte0, NB, vec != 0) ^ flip;
            lo += w & 0x0F0F0F0Fu, hi += (w >> 4) & 0x0F0F0F0Fu;
            if (++rows == 17) widen();      // 17 * 15 = 255: a byte is full
        }
        widen();
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) part[ph][8 * cg + b] = s[b];
    __syncthreads();
    if (threadIdx.x < kBN) {
        uint32_t total = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) total += part[i][threadIdx.x];
        const uint32_t n = blockIdx.x * kBN + threadIdx.x;
        if (n < N) {
            const uint32_t z = ((zp ? static_cast<uint32_t>(zp[per_column ? n : 0u]) : 0u) ^ flip) & 0xFu;
            sums[static_cast<int64_t>(blockIdx.y) * stride + n] = static_cast<int32_t>(total - (k_end - k_begin) * z);
        }
    }
}

bool request_ok(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    return shape_ok(M, K, N) && K <= kMaxK && N % 2 == 0 && (x_mode == OQ_QDQ_STATIC || x_mode == OQ_QDQ_DYNAMIC) && mode_ok(out_mode);
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

int32_t oq_qdq_function_packed4_extension_version(void) { return OQ_QDQ_FUNCTION_PACKED4_EXTENSION_VERSION; }

size_t oq_qdq_function_packed4_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode, int32_t out_mode) {
    if (!request_ok(M, K, N, x_mode, out_mode)) {
        set_error("oq_qdq_function_packed4_workspace_bytes: M=%lld K=%lld N=%lld x_mode=%d out_mode=%d outside the bounds (K <= %lld, an even N)",
                  (long long)M, (long long)K, (long long)N, x_mode, out_mode, (long long)kMaxK);
        return 0;
    }
    Workspace ws(/* aligned_base */ true);
    make_qdq_function_plan(M, K, N, x_mode, out_mode, ws);
    return ws.total();
}

int32_t oq_qdq_function_packed4(const void* X, int32_t atype, int64_t M, int64_t K, int64_t lda, int32_t x_mode, int32_t x_type, const float* x_scale,
                                const void* x_zero_point, const void* W, int32_t wtype, int64_t N, int64_t ldw, int32_t granularity,
                                int64_t group_size, const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale,
                                const int32_t* b_zero_point, int32_t out_mode, int32_t out_type, const float* out_scale, const void* out_zero_point,
                                float* Y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "oq_qdq_function_packed4";
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
    const QdqFunctionPlan pl = make_qdq_function_plan(M, K, N, x_mode, out_mode, ws);
    OQ_REQUIRE(ws.fits(), OQ_ERR_WORKSPACE, "%s: a 256-byte aligned workspace of %zu bytes is needed, %zu given", fn, ws.total(),
               workspace ? workspace_bytes : (size_t)0);

    hipStream_t s = as_stream(stream);
    Packed4FnArgs p{};      // the epilogue's B: signed, no zero point -- W's zero points are subtracted in the staging
    const float* const quant_scale = fill_qdq_args(p, pl, M, K, x_mode, x_type, x_scale, x_zero_point, W, OQ_QL_I8, N, ldw, w_scale, nullptr,
                                                   granularity == OQ_CHANNEL, B, b_scale, b_zero_point, out_mode, out_type, out_scale, out_zero_point,
                                                   Y, ldy);
    p.b_vec = aligned_to(W, 4) && ldw % 4 == 0;
    p.w_zp = static_cast<const uint8_t*>(w_zero_point), p.w_per_column = granularity == OQ_CHANNEL;
    p.nibble_flip = wtype == OQ_INT4 ? 0x88888888u : 0u;
    return run_qdq_function(p, pl, static_cast<const float*>(X), lda, quant_scale, Y, ldy, s, [&]() -> int32_t {
        if (p.colsum) {
            qp_sum_cols_kernel<<<dim3(static_cast<unsigned>(ceil_div(N, kBN)), kColSlices), kThreads, 0, s>>>(
                p.B, p.K, p.N, ldw, p.b_vec, p.nibble_flip, p.w_zp, p.w_per_column, pl.colsum, p.colsum_stride);
            const int32_t st = check_launch("qp_sum_cols_kernel");
            if (st != OQ_OK) return st;
        }
        const dim3 grid(static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.splits));
        with_row_tiles(pl, [&](auto mt) { qp_gemm_kernel<decltype(mt)::value><<<grid, kThreads, 0, s>>>(p); });
        return check_launch("qp_gemm_kernel");
    });
}

}  // extern "C"
