/*
 * oq_hip_half.h -- half-precision extension of the C ABI of oq_hip.h: RTN, HQQ and the AWQ / SmoothQuant searches on fp16 / bf16
 * weights, the GPTQ Hessian and the calibration statistics (running min / max, absmax, the |x| column statistics of the AWQ /
 * SmoothQuant searches) of fp16 / bf16 activations, all read as they are.
 *
 * oq_hip.h stays what it is (OQ_ABI_VERSION 2); the entry points below live in the same library and follow the same
 * conventions (device pointers, asynchronous on `stream`, no allocation, 0 or a negative oq_status, oq_last_error()).
 * Both conversions to fp32 are exact, so every result is DEFINED as that of the fp32 entry point on the upcast matrix:
 * the integers, zero points and fp32 scales of RTN match it bit for bit; the Hessian (a sum, whose order is the kernel's own)
 * is held to the same tolerance against float64 as the fp32 entry point.
 */
#ifndef OQ_HIP_HALF_H
#define OQ_HIP_HALF_H

#include "oq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_HALF_EXTENSION_VERSION 1

/* element type of a 2-byte matrix (weights, activations) */
typedef enum { OQ_W_F16 = 0 /* IEEE binary16 */, OQ_W_BF16 = 1 /* bfloat16 */ } oq_wtype;

/* OQ_HALF_EXTENSION_VERSION of the loaded library */
int32_t oq_half_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 * A1  core/_algorithms/rtn.py:54-109  _rtn_quantize on W.astype(np.float32), without the fp32 copy: replaces the cast
 *     followed by oq_rtn_quantize_f32 with mse == 0 (mse == 1: oq_rtn_mse_h16 below).
 *
 *   W          [K, N], 2 bytes per element of type `wtype`, leading dimension ldw >= N (elements).  Rows that are not
 *              16-byte aligned (odd N, odd ldw, an unaligned base) take narrower loads and give the same bytes.
 *   group_size GROUP only: > 0 (clamped to K), or -1 (= K); K % group_size must be 0 (groups that straddle columns:
 *              OQ_ERR_UNSUPPORTED -- cast and call oq_rtn_quantize_f32).
 *   q_out      OQ_LAYOUT_KN: K*N bytes.  OQ_LAYOUT_NBITS: N*(K/g)*(g*bits/8) bytes (group strategy, g % 16 == 0,
 *              16-byte aligned).  OQ_LAYOUT_KN_PACKED4: OQ_ERR_UNSUPPORTED -- quantize to OQ_LAYOUT_KN and pack with
 *              oq_pack_nibbles.  NULL: parameters only (what oq_rtn_qparams_f32 does for fp32).
 *   scale_out  fp32, zp_out 1 byte each: exactly the arrays of oq_rtn_quantize_f32 (group: entry n*(K/g)+kg).
 *   workspace  oq_rtn_half_workspace_bytes: 0 for groups of up to 256 rows (one fused launch, W read once); channel,
 *              tensor and taller groups run a range pass and a quantize pass over W and keep the partial ranges there
 *              (4-byte aligned).  The query returns 0 for a request outside the bounds of oq_hip.h as well.
 * ------------------------------------------------------------------------------------------- */
size_t oq_rtn_half_workspace_bytes(int64_t K, int64_t N, int32_t strategy, int64_t group_size);
int32_t oq_rtn_quantize_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype,
                            int32_t strategy, int64_t group_size, int32_t symmetric, int32_t reduce_range,
                            float clip_ratio, void* q_out /* NULL: parameters only */, float* scale_out,
                            void* zp_out, int32_t layout, void* workspace, size_t workspace_bytes, void* stream);

/* A1 with the MSE range search (utils.py:140-239): _rtn_quantize(..., mse=True) on W.astype(np.float32), without the fp32 copy:
 *     replaces the cast followed by oq_rtn_quantize_f32 / oq_rtn_qparams_f32 with mse == 1.  Both conversions are exact and the
 *     search arithmetic stays fp32 -- per element, per candidate and in the order of every sum that of the fp32 kernels -- so the
 *     result is DEFINED as that of the fp32 entry points on the upcast matrix: integers, zero points and fp32 scales match it
 *     byte for byte, NaN patterns included.
 *
 *   W          [K, N], 2 bytes per element of type `wtype`, leading dimension ldw >= N (elements), 2-byte aligned; no other
 *              alignment is needed (every lane reads its own column, 2 bytes a row).
 *   routes     those of the fp32 search: group_size 32 / 64 / 128 hold a group in registers across the 20 candidates (converted
 *              at the load); every other group size, channel and tensor re-read W per candidate.  group_size 256: the register
 *              route as well, the group held as PACKED 2-byte elements (128 registers) -- fp32 has no such route.
 *   group_size GROUP only: > 0 (clamped to K), or -1 (= K); K % group_size must be 0 (groups that straddle columns:
 *              OQ_ERR_UNSUPPORTED, as with mse in oq_rtn_quantize_f32).
 *   clip_ratio validated, then not applied: the MSE range replaces the clipped one, as in oq_rtn_quantize_f32 with mse.
 *   q_out      OQ_LAYOUT_KN only: K*N bytes, or NULL: parameters only.  OQ_LAYOUT_NBITS / OQ_LAYOUT_KN_PACKED4:
 *              OQ_ERR_UNSUPPORTED, as the fp32 entry points answer with mse.
 *   scale_out  fp32, 4-byte aligned; zp_out 1 byte each: the arrays of oq_rtn_quantize_f32 (group: entry n*(K/g)+kg).
 *   workspace  oq_rtn_mse_half_workspace_bytes (4-byte aligned): 12 bytes per (scale, zp) pair + 82432.  The query returns 0
 *              and sets the error for a request outside the bounds, like oq_rtn_half_workspace_bytes.
 *   checks     null pointers, wtype, alignment, the shape bounds, clip_ratio, the layout, the group and the workspace, all
 *              before the first device call: on any refusal no output is touched. */
size_t oq_rtn_mse_half_workspace_bytes(int64_t K, int64_t N, int32_t strategy, int64_t group_size);
int32_t oq_rtn_mse_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype, int32_t strategy,
                       int64_t group_size, int32_t symmetric, int32_t reduce_range, float clip_ratio,
                       void* q_out /* NULL: parameters only */, float* scale_out, void* zp_out, int32_t layout,
                       void* workspace, size_t workspace_bytes, void* stream);

/* A1 over a LIST of equally shaped 2-byte matrices of ONE element type that live anywhere in device memory (the MatMul weights of
 *     a resident fp16 / bf16 model): what oq_rtn_quantize_ptrs_f32 (oq_hip.h) is for fp32 weights.  Entry i of the table holds the
 *     four device pointers of matrix i; all matrices of a call share K, N, ldw, the group size and the quantization grid.
 *
 *   scope      the group strategy with K % group_size == 0 and group_size <= 256 (after the clamp to K; -1 = K): exactly what
 *              oq_rtn_quantize_h16 runs as one fused launch.  Everything else OQ_ERR_UNSUPPORTED -- call oq_rtn_quantize_h16 per
 *              matrix.  No workspace, no state: no workgroup waits for another, nothing is accumulated.
 *   result     per matrix that of oq_rtn_quantize_h16, bit for bit (and so that of oq_rtn_quantize_f32 on the upcast matrix).
 *   tables     `table_host` and `table_device` are the same `count` entries in host and device memory: the host copy is checked
 *              and sizes the launches, the kernels read the device copy, which may be NULL when count == 1.  1 <= count <= 65535.
 *              About 1.6e8 parameters share a launch (blockIdx.y = entry, at most 65535), the rule of oq_rtn_quantize_ptrs_f32;
 *              later launches read table_device + i.
 *   W          [K, N] of type `wtype`, leading dimension ldw >= N (elements), 2-byte aligned.
 *   q_out      OQ_LAYOUT_KN: K*N bytes.  OQ_LAYOUT_NBITS: the blob, group_size % 16 == 0 and every q_out 16-byte aligned.
 *              OQ_LAYOUT_KN_PACKED4: K*N/2 bytes, two columns per byte in core/_pack.py:8-22 order -- the bytes oq_pack_nibbles
 *              makes of the [K, N] result, without the [K, N] store, the packer's read and its launch; 4-bit types, even N and a
 *              group_size of 16 / 32 / 64 / 128 / 256 (OQ_ERR_UNSUPPORTED otherwise).  Never NULL.
 *   scale_out  fp32, 4-byte aligned; zp_out 1 byte each: entry n*(K/g)+kg, as in oq_rtn_quantize_h16.
 *   widths     16-byte loads of W need N % 8 == 0, ldw % 8 == 0 and EVERY W 16-byte aligned; whole 8-byte ([K, N]) or 4-byte
 *              ([K, N/2]) stores need N % 8 == 0 and EVERY q_out aligned to them.  One entry short of that puts the whole call on
 *              the narrow build, which gives the same bytes: group entries by alignment where that matters.
 *   checks     an unknown wtype, null tables, count, the shape bounds, clip_ratio, the layout rules and, entry by entry, null
 *              pointers and alignment (the message names the entry) -- all on the host copy before anything is launched: on any
 *              refusal no output is touched. */
typedef struct {
    const void* W;
    void* q_out;
    float* scale_out;
    void* zp_out;
} oq_rtn_ptrs_h16;   /* the layout of oq_rtn_ptrs */
int32_t oq_rtn_quantize_ptrs_h16(const oq_rtn_ptrs_h16* table_host, const oq_rtn_ptrs_h16* table_device, int64_t count,
                                 int32_t wtype, int64_t K, int64_t N, int64_t ldw, int32_t qtype, int64_t group_size,
                                 int32_t symmetric, int32_t reduce_range, float clip_ratio, int32_t layout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2  core/_algorithms/hqq.py:106-213  optimize_weights + the final quantization on W.astype(np.float32), without the fp32
 *     copy: replaces the cast followed by oq_hqq_optimize_f32 (oq_hip.h).  Both conversions to fp32 are exact and the
 *     arithmetic of HQQ stays fp32, so the result is DEFINED as that of oq_hqq_optimize_f32 on the upcast matrix: the integers
 *     (both layouts), the float zero points and `rounds` match it bit for bit on every route.  The kernels keep the fp32
 *     kernels' work split (one thread per (column, k-group), 256 columns per block), so the float64 partial sums of
 *     |w - w_r|, their fold and with them every `best` / early-stop decision are the same.
 *
 *   W          [K, N], 2 bytes per element of type `wtype`, leading dimension ldw >= N (elements), 2-byte aligned; no other
 *              alignment is needed (every lane reads its own column, 2 bytes a row).
 *   routes     group_size 16 / 32 / 64 / 128 and 1 <= iters <= 32: all rounds in one pass over W, a group's values held in
 *              registers as fp32 (three launches), as for fp32.  group_size 256: the same one pass, the group held as
 *              PACKED 2-byte elements (128 registers) -- oq_hqq_optimize_f32 has no such route and re-reads W every round.
 *              Everything else, and per_round_launches != 0: one launch pair per round (2 * iters + 1 launches).
 *   arguments  every other argument, the workspace (oq_hqq_workspace_bytes, 8-byte aligned), the statuses and the messages
 *              are those of oq_hqq_optimize_f32; in addition an unknown wtype and a W that is not 2-byte aligned are
 *              OQ_ERR_INVALID_ARGUMENT.  Everything is refused on the host before any launch: no output is touched.
 * ------------------------------------------------------------------------------------------- */
int32_t oq_hqq_optimize_h16(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw /* elements */, int64_t group_size,
                            int32_t reduce_range, const float* scale, const float* zero_point_in, double lp_norm, double beta,
                            double kappa, int32_t iters, int32_t early_stop, int32_t per_round_launches, void* q_out, int32_t layout,
                            float* zero_point_out, int32_t* rounds_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * G1  core/_algorithms/gptq.py:246-260  _accumulate_hessian on inp.astype(np.float32) (:257), without the fp32 copy:
 *     replaces the cast followed by oq_hessian_accumulate_f32.
 *
 *       H <- H * n_seen / (n_seen + n_add) + 2 / (n_seen + n_add) * X^T X        on the exact fp32 values of X
 *
 *   X          [T, K], 2 bytes per element of type `xtype` (an oq_wtype), leading dimension ldx >= K (elements).  Rows that
 *              are only 2-byte aligned (odd ldx, an unaligned base) take narrower loads and give the same result.
 *   H          fp32 [K, K], contiguous; comes out full and exactly symmetric.  n_add: the sample count (gptq.py:247), not T.
 *   method     there is none: an fp16 x fp16 or bf16 x bf16 product is exact in fp32, so every pair of elements meets in
 *              ONE matrix-core product (v_mfma_f32_16x16x32_f16 / _bf16, fp32 accumulation) with no split, no scale and no
 *              product rounding; only the order of the fp32 sums differs from float64.  At least as exact as every method
 *              of oq_hessian_accumulate_f32.
 *   route      one route for every T >= 1, K >= 1 (K <= 2^17, T * ldx <= 2^40 as in oq_hip.h): a re-layout kernel packs
 *              eight rows of a column into 16 bytes (2 B read, 2 B written per element, zero padding to 32 rows and 256
 *              columns; X is never expanded to fp32 in memory), then 256 x 256 tiles of the upper triangle.  From 993 rows
 *              (two slices of >= 512 rows after padding to 32) T is cut into up to 16 slices where that fills the 256
 *              CUs better, the slices are summed in slice order (deterministic) -- slab permitting: the query budgets 16
 *              slabs of K x K floats for K <= 8192 and 4 above, a smaller workspace gets fewer slices.
 *   workspace  oq_hessian_half_workspace_bytes(T, K): the packed operand and the slabs.  At least the packed operand
 *              (T padded to 32 x K padded to 256 x 2 bytes, + 256) must be given: OQ_ERR_WORKSPACE otherwise, H untouched.
 *              The query returns 0 for a request outside the bounds.
 * ------------------------------------------------------------------------------------------- */
size_t oq_hessian_half_workspace_bytes(int64_t T, int64_t K);
int32_t oq_hessian_accumulate_h16(const void* X, int32_t xtype /* oq_wtype */, int64_t T, int64_t K, int64_t ldx, int64_t n_seen,
                                  int64_t n_add, float* H, void* workspace, size_t workspace_bytes, void* stream);

/* G1 for a LIST of 2-byte inputs of ONE element type in one launch chain: what oq_hessian_accumulate_many_f32 (oq_hip.h) is
 *     for fp32 inputs -- the tensors one calibration batch taps, each far too small to fill the device alone.  Every item is one
 *     oq_hessian_accumulate_h16 call; the chain is three launches for the whole table (plan, re-layout, product) whose blocks
 *     never wait for one another.
 *
 *   items      `count` oq_hessian_item (oq_hip.h, unchanged) in host memory and the same bytes in device memory: the host copy
 *              is checked and sizes the launches, the kernels read the device copy.  `X` points at 2-byte elements of type
 *              `xtype` (2-byte aligned, ldx >= K in elements); every other field as in oq_hip.h.  Items whose rows are only
 *              2-byte aligned (odd ldx, an unaligned base) take narrower loads, item by item, and give the same result.
 *              1 <= count <= 65535.
 *   H          of every item: fp32 [K, K], contiguous, comes out full and exactly symmetric; read only when n_seen > 0.
 *   result     every item runs ONE T-slice: an item of up to 992 rows (where oq_hessian_accumulate_h16 runs one slice too)
 *              gets the bits of that call.  A longer item is summed in one fp32 chain where the per-tensor call slices T
 *              from 993 rows: the same tolerance against float64, not the same bits.
 *   checks     the bounds of oq_hessian_accumulate_h16 for every item (OQ_ERR_INVALID_ARGUMENT / OQ_ERR_UNSUPPORTED, the
 *              message names the item), an unknown xtype OQ_ERR_INVALID_ARGUMENT, a missing or short workspace
 *              OQ_ERR_WORKSPACE -- all on the host copy before anything is launched: on any refusal no H is touched.
 *   workspace  oq_hessian_many_half_workspace_bytes(items_host, count) =
 *                  count * 128 (the device table) rounded up to 256
 *                + the packed operand of every item: T padded to 32 x K padded to 256 x 2 bytes
 *                + 512.
 *              The query returns 0 for a table outside the bounds (null, count, T, K of an item). */
size_t oq_hessian_many_half_workspace_bytes(const oq_hessian_item* items_host, int64_t count);
int32_t oq_hessian_accumulate_many_h16(const oq_hessian_item* items_host, const oq_hessian_item* items_device, int64_t count,
                                       int32_t xtype /* oq_wtype */, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * C1  core/_calibration/minmax.py:40-64  MinMaxCalibrator.collect on x.astype(np.float32), without the fp32 copy: replaces
 *     the cast followed by oq_minmax_collect_f32.  Min and max of fp16 / bf16 values are exact, so `state` comes out as
 *     oq_minmax_collect_f32 leaves it on the upcast tensor, bit for bit (NaN anywhere -> both extrema NaN, -0 < +0,
 *     subnormals are values).
 *
 *   x          `count` elements of 2 bytes of type `xtype` (an oq_wtype), 2-byte aligned: the elements in front of the first
 *              16-byte boundary and behind the last one are read singly, the rest eight at a time.
 *   state      fp32 {min, max, seen, -} in device memory, as in oq_minmax_collect_f32 (zero-filled before its first use).
 *   momentum   in [0, 1): 0 keeps the running min / max, > 0 the EMA of minmax.py:53-60.
 *   workspace  oq_minmax_half_workspace_bytes (4-byte aligned).  The query returns 0 for a count outside 1 .. 2^40.
 * ------------------------------------------------------------------------------------------- */
size_t oq_minmax_half_workspace_bytes(int64_t count);
int32_t oq_minmax_collect_h16(const void* x, int32_t xtype /* oq_wtype */, int64_t count, float* state, double momentum,
                              void* workspace, size_t workspace_bytes, void* stream);

/* C1 for a whole calibration batch of 2-byte tensors of ONE element type: replaces a cast and an oq_minmax_collect_f32 per
 *     tensor (calibrate.py:264-266) by one launch pair, as oq_minmax_collect_many_f32 does for fp32 tensors.  `desc` is a
 *     DEVICE array (8-byte aligned) of n oq_minmax_desc {x, count, state} whose `x` points at 2-byte elements of type
 *     `xtype`; every count > 0; each state fp32 as above.  1 <= n <= 65535; the query returns 0 outside. */
size_t oq_minmax_many_half_workspace_bytes(int64_t n);
int32_t oq_minmax_collect_many_h16(const void* desc, int64_t n, int32_t xtype /* oq_wtype */, double momentum, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * S1  pre_passes/smooth_quant.py:62-74  the per-channel max |x| on x.astype(np.float32), without the fp32 copy: replaces the cast followed by oq_absmax_f32.  |x| of an fp16 / bf16 value is exact: `out` equals
 *     oq_absmax_f32's on the upcast matrix bit for bit (starting from 0; a NaN poisons exactly its column / row).
 *
 *   x          [R, C], 2 bytes per element of type `xtype` (an oq_wtype), leading dimension ldx >= C (elements).  Rows that
 *              are not 16-byte aligned (C or ldx no multiple of 8, an unaligned base) take 2-byte loads and give the same.
 *   transposed 0: out[c] = max_r |x[r, c]| (C floats).  Non-zero: out[r] = max_c |x[r, c]| (R floats), no workspace used.
 *   workspace  oq_absmax_half_workspace_bytes (4-byte aligned): the per-128-row partial maxima.  The query returns 0 for a
 *              shape outside the bounds of oq_hip.h.
 * ------------------------------------------------------------------------------------------- */
size_t oq_absmax_half_workspace_bytes(int64_t R, int64_t C, int32_t transposed);
int32_t oq_absmax_h16(const void* x, int32_t xtype /* oq_wtype */, int64_t R, int64_t C, int64_t ldx, int32_t transposed, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2s pre_passes/awq.py:47-50 (sum_t |x[t, k]|) and pre_passes/smooth_quant.py:62-69 (max_t |x[t, k]|) as RUNNING statistics
 *     over calibration batches, for a LIST of 2-byte inputs of ONE element type, without an fp32 copy: replaces, per tensor, the
 *     cast, oq_abs_sum_cols_f32(accumulate = 1), oq_absmax_f32 and the maximum with the running value.  Each input is read
 *     once for both statistics; the whole table takes two launches (partials, fold) whose blocks never wait for one another;
 *     no atomics.
 *
 *   items      `count` oq_abs_stats_item in host memory and the same bytes in device memory (8-byte aligned): the host copy is
 *              checked and sizes the launches, the kernels read the device copy, which may be NULL when count == 1.
 *              1 <= count <= 65535.
 *   X          [T, K], 2 bytes per element of type `xtype`, leading dimension ldx >= K (elements), 2-byte aligned.  Items whose
 *              rows are not 16-byte aligned (K or ldx no multiple of 8, an unaligned base) take narrower loads, item by item,
 *              and give the same bits.
 *   abs_sum    fp32 [K], 4-byte aligned:  abs_sum[k] <- abs_sum[k] + S_k, S_k the sum over the rows of |x[t, k]| on the exact
 *              fp32 values in the order of oq_abs_sum_cols_f32 (min(T, 64) row chunks of ceil(T / chunks) rows; inside a chunk
 *              fours as (a + b) + (c + d), then single rows; the chunks added from 0): the bits of
 *              oq_abs_sum_cols_f32(..., accumulate = 1) on the upcast matrix.
 *   absmax     fp32 [K], 4-byte aligned:  absmax[k] <- max(absmax[k], max_t |x[t, k]|), NaN-propagating (a NaN in the running
 *              value or in the column gives NaN): the maximum of the running value and oq_absmax_f32 on the upcast matrix.
 *   checks     an unknown xtype, null tables, count and, item by item, null pointers, alignment and the extent rules of oq_hip.h
 *              (T, K >= 1, ldx >= K, all < 2^31, T * ldx <= 2^40) OQ_ERR_INVALID_ARGUMENT (the message names the item); a missing
 *              or short workspace OQ_ERR_WORKSPACE -- all on the host copy before anything is launched: on any refusal no
 *              output is touched.
 *   workspace  oq_abs_stats_many_half_workspace_bytes(items_host, count) =
 *                  count * max over the items of (min(T, 64) * K) * 8   (the partial sums and maxima, one slot per item)
 *                + 256.
 *              The query returns 0 for a table outside the bounds (null, count, T, K, ldx of an item).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const void* X;
    int64_t T, K, ldx;
    float* abs_sum;
    float* absmax;
} oq_abs_stats_item;
size_t oq_abs_stats_many_half_workspace_bytes(const oq_abs_stats_item* items_host, int64_t count);
int32_t oq_abs_stats_cols_many_h16(const oq_abs_stats_item* items_host, const oq_abs_stats_item* items_device, int64_t count,
                                   int32_t xtype /* oq_wtype */, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2h pre_passes/awq.py:114-184 (scale search), :207-259 (clip search) and pre_passes/smooth_quant.py:62-74, :111-113 on
 *     W.astype(np.float32), without the fp32 copy: replace the cast followed by oq_awq_scale_search_f32,
 *     oq_awq_clip_search_f32, oq_awq_scale_search_stats_f32, oq_awq_clip_search_stats_f32 and oq_smooth_quant_scale_f32
 *     (oq_hip.h).  A search reads W once per candidate (20 + 10 passes) and for its weight statistics; every one of those
 *     reads takes the 2-byte matrix as it is and converts at the load.  Both conversions are exact, every lane owns the
 *     elements it owns in the fp32 kernels and every sum keeps its order, so the result is DEFINED as that of the `_f32`
 *     entry point on the upcast matrix: `scales_out` (all n_grid rows), `losses_out`, `best_out` and `scale_out` match it
 *     byte for byte, NaN patterns included.
 *
 *   arguments  those of the `_f32` twins, with `const void* W, int32_t wtype` in place of `const float* W`.  X, act_sum and G
 *              stay fp32 (half activations become statistics through N2s and oq_hessian_accumulate_h16).
 *   W          [K, N], 2 bytes per element of type `wtype`, leading dimension ldw >= N (elements), 2-byte aligned.
 *              N % 4 == 0, ldw % 4 == 0 and an 8-byte aligned base give 8-byte loads (four elements) on the fused group
 *              kernel, the four-column difference kernel and the row-scale kernel; anything else -- rows that are only
 *              2-byte aligned are legal -- takes the one-column kernels and gives the same bytes.
 *   routes     those of the fp32 searches.  The general route quantizes through the fp32 RTN: for the scale search on the
 *              candidate's scaled weights, which are written as fp32 from the 2-byte W (as for fp32); for the clip search
 *              on W itself, through oq_rtn_quantize_h16 -- no fp32 copy of W exists on any route.
 *   workspace  256-byte aligned.
 *                oq_awq_half_workspace_bytes(T, K, N)     = oq_awq_workspace_bytes(T, K, N)     + R(K, N)
 *                oq_awq_stats_half_workspace_bytes(K, N)  = oq_awq_stats_workspace_bytes(K, N)  + R(K, N)
 *                R(K, N) = 8 * N * (ceil(K / 64) + K / 257 + 1) rounded up to 256, + 256
 *              (R: the partial ranges of oq_rtn_quantize_h16 for channel, tensor and groups of more than 256 rows, behind the
 *              fp32 layout).  Both return 0 where the fp32 query returns 0 (a shape outside the bounds, K > 65535).
 *              oq_smooth_quant_scale_h16 takes oq_smooth_quant_workspace_bytes(K), as its twin.
 *   checks     an unknown wtype and a W that is not 2-byte aligned OQ_ERR_INVALID_ARGUMENT; then every refusal of the twin
 *              with its status (n_grid outside 1 .. 64, a group below 4 or one that does not divide K, K > 65535, a
 *              missing, short or misaligned workspace, null pointers) -- all on the host before the first launch: on any
 *              refusal no output is touched.
 * ------------------------------------------------------------------------------------------- */
size_t oq_awq_half_workspace_bytes(int64_t T, int64_t K, int64_t N);
size_t oq_awq_stats_half_workspace_bytes(int64_t K, int64_t N);
int32_t oq_awq_scale_search_h16(const float* X, int64_t T, int64_t K, int64_t ldx, const void* W, int32_t wtype, int64_t N,
                                int64_t ldw, int32_t qtype, int32_t strategy, int64_t group_size, int32_t symmetric,
                                int32_t reduce_range, int32_t n_grid, float* scales_out /* [n_grid, K] */, float* losses_out,
                                int32_t* best_out, void* workspace, size_t workspace_bytes, void* stream);
int32_t oq_awq_clip_search_h16(const float* X, int64_t T, int64_t K, int64_t ldx, const void* W, int32_t wtype, int64_t N,
                               int64_t ldw, int32_t qtype, int32_t strategy, int64_t group_size, int32_t symmetric,
                               int32_t reduce_range, float* losses_out /* [10] */, int32_t* best_out, void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t oq_awq_scale_search_stats_h16(const float* act_sum, const float* G, int64_t T, int64_t K, const void* W, int32_t wtype,
                                      int64_t N, int64_t ldw, int32_t qtype, int32_t strategy, int64_t group_size,
                                      int32_t symmetric, int32_t reduce_range, int32_t n_grid, float* scales_out,
                                      float* losses_out, int32_t* best_out, void* workspace, size_t workspace_bytes,
                                      void* stream);
int32_t oq_awq_clip_search_stats_h16(const float* G, int64_t T, int64_t K, const void* W, int32_t wtype, int64_t N, int64_t ldw,
                                     int32_t qtype, int32_t strategy, int64_t group_size, int32_t symmetric,
                                     int32_t reduce_range, float* losses_out, int32_t* best_out, void* workspace,
                                     size_t workspace_bytes, void* stream);
int32_t oq_smooth_quant_scale_h16(const float* X, int64_t T, int64_t K, int64_t ldx, const void* W, int32_t wtype, int64_t N,
                                  int64_t ldw, float alpha, float* scale_out, void* workspace, size_t workspace_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_HALF_H */
