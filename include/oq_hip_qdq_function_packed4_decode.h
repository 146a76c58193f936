/*
 * oq_hip_qdq_function_packed4_decode.h -- extension of the C ABI of oq_hip.h: the decode route of oq_hip_qdq_function_packed4.h.  The
 * same call -- one `quant`-domain QDQ function with QUANTIZED ACTIVATIONS, fp32 X in, fp32 Y out, a 4-bit weight as the [K, N / 2]
 * packed nibbles the file stores -- for 1 ... 16 rows of X, where the weight is all the traffic there is: W is read ONCE, straight
 * from global memory into the registers that feed v_mfma_i32_16x16x64_i8, with no tile to pad to.
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and the other extensions stay what they are; nothing is rerouted: oq_qdq_function_packed4 takes every
 * M, this entry point only M <= 16.  Conventions: those of oq_hip_qdq_function_packed4.h -- device pointers only, asynchronous on
 * `stream`, no allocation, no host synchronisation, capturable into a HIP graph, no atomics, deterministic; 0 or a negative
 * oq_status, oq_last_error().  Every refusal happens on the host before the first launch: no output is touched.  EVERY PARAMETER IS
 * READ ON THE DEVICE.
 *
 * Arithmetic: the block of oq_hip_qdq_function.h, step for step, with the nibble rule of oq_hip_qdq_function_packed4.h.  The result
 * is THE SAME BYTES as oq_qdq_function_packed4 for every accepted call: both form the exact int32
 *       S = sum_k (q_x - 128 [uint8]) (W - zp_w) - zp_x' * sum_k (W - zp_w)[n],           zp_x' = zp_x - 128 [uint8]
 * (uint32 arithmetic, any order of the partial sums gives the same bits) and run the same epilogue text on it.
 *
 * What runs (csrc/qdq_function_packed4_decode.hip):
 *   product      one kernel for every M <= 16.  A workgroup takes 128 columns and one slice of K; it quantizes its slice of X into LDS
 *                (the static quantizer, or the parameters the launches in front left on the device), and each of its four waves
 *                multiplies a quarter of the slice.  In a wave the 16-lane group g = lane >> 4 walks the rows 64 s + 16 g ... + 15 of
 *                a 64-k span and lane & 15 loads one dword -- 8 columns -- of each: after the nibble split, the byte-wise W - zp_w
 *                and the 4 x 4 byte transposes the lane holds, for each of its 8 columns, the 16 consecutive k that are exactly its
 *                share of the matrix instruction's B operand.  No LDS and no cross-lane traffic for W.  The column sums come from one
 *                more matrix instruction per operand, against a fragment of ones; they are left out where zp_x' is zero whatever
 *                the device holds (a static int8 X with a NULL zero point).
 *   launches     static input:  product [, reduce of the K slices] [, finish of a dynamic output]: static / none is at most two.
 *                dynamic input: min / max of X, its parameters, then the same: three to five.
 *                splits == 1 (one slice of K): the product launch finishes Y itself.
 *   plan         slice  = min(2048, ceil(ceil(K / want) / 64) * 64), want = ceil((M <= 4 ? 512 : 256) / ceil(N / 128))
 *                splits = ceil(K / slice)
 *
 * Left out, deliberately: what oq_hip_qdq_function_packed4.h leaves out (an odd N, grouped W, fp16 / bf16 X, packed zero points), and
 *   M > 16                        OQ_ERR_UNSUPPORTED, by name: oq_qdq_function_packed4 is the entry point for such a call.
 *   a dot4 tier for M <= 4        the vector work per weight does not depend on M; the matrix instruction is not the issue-rate term.
 */
#ifndef OQ_HIP_QDQ_FUNCTION_PACKED4_DECODE_H
#define OQ_HIP_QDQ_FUNCTION_PACKED4_DECODE_H

#include "oq_hip_qdq_function_packed4.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_FUNCTION_PACKED4_DECODE_EXTENSION_VERSION 1

/* OQ_QDQ_FUNCTION_PACKED4_DECODE_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_function_packed4_decode_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   every argument as in oq_qdq_function_packed4 (oq_hip_qdq_function_packed4.h), with 1 <= M <= 16.  K <= 561433; N counts values
 *   and is even; ldw >= N / 2 counts BYTES; any byte alignment of W's base and rows (4-byte aligned rows take dword loads and give
 *   the same bytes).  No byte outside [K, N / 2] of W and no float of X at or beyond column K is read.
 *   workspace    256-byte aligned.  oq_qdq_function_packed4_decode_workspace_bytes(M, K, N, x_mode, out_mode) is the sum, each piece
 *                rounded up to 256 bytes, of
 *                  S   splits > 1: splits * M * N * 4, the int32 slabs of the K slices                     (plan: above)
 *                  P   a dynamic input: 12, its parameters (safe, scale, zp)
 *                  PX  a dynamic input: ceil(M / 4) * 8, the (min, max) pairs of the pass over X
 *                  PO  a dynamic output: 8 for every workgroup that finishes Y: ceil(N / 128) of them for splits == 1, else
 *                      ceil(M * N / 256)
 *                `workspace` may be NULL where the sum is 0.  The query returns 0 (and sets oq_last_error) for a request outside
 *                the bounds, with an unknown mode, with an odd N or with M > 16.
 *   checks       those of oq_qdq_function_packed4 with the same status codes; M > 16 OQ_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_function_packed4_decode_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode /* oq_qdq_mode */,
                                                      int32_t out_mode /* oq_qdq_mode */);
int32_t oq_qdq_function_packed4_decode(const void* X, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, int32_t x_mode /* oq_qdq_mode */,
                                int32_t x_type /* oq_ql_type */, const float* x_scale, const void* x_zero_point, const void* W,
                                int32_t wtype /* OQ_UINT4 | OQ_INT4 */, int64_t N, int64_t ldw /* bytes */, int32_t granularity /* oq_strategy */,
                                int64_t group_size, const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale,
                                const int32_t* b_zero_point, int32_t out_mode /* oq_qdq_mode */, int32_t out_type /* oq_ql_type */,
                                const float* out_scale, const void* out_zero_point, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_FUNCTION_PACKED4_DECODE_H */
