/*
 * oq_hip_qdq_function_packed4.h -- extension of the C ABI of oq_hip.h: the call of oq_hip_qdq_function.h -- one `quant`-domain QDQ
 * function with QUANTIZED ACTIVATIONS, fp32 X in, fp32 Y out, the product on the int8 matrix cores -- run from a 4-bit weight as
 * the file stores it: an ONNX INT4 / UINT4 initializer [K, N], two values per byte in flat order, the even index in the low nibble
 * (what OQ_LAYOUT_KN_PACKED4 of oq_hip.h writes on the quantize side, and what oq_hip_qdq_packed4.h reads for the fp16-piece
 * product).  oq_qdq_function reads such a weight only after it has been unpacked to one value per byte; the entry point below reads
 * the bytes as stored: half the memory and half the weight read.
 *
 * oq_hip.h (OQ_ABI_VERSION 2) and the other extensions stay what they are; nothing is rerouted.  The entry points below live in the
 * same library and follow the conventions of oq_hip_qdq_function.h: device pointers only, asynchronous on `stream`, no allocation,
 * no host synchronisation, capturable into a HIP graph, no atomics, deterministic; 0 or a negative oq_status, oq_last_error().
 * Every refusal happens on the host before the first launch: no output is touched.  EVERY PARAMETER IS READ ON THE DEVICE.
 *
 * Arithmetic: the block of oq_hip_qdq_function.h, step for step, with
 *       W[k, n] = nibble (n & 1) of byte W[k * ldw + n / 2]          (OQ_INT4: the nibble's two's-complement value)
 * For K <= 33025 the result is THE SAME BYTES as oq_qdq_function on the same weight unpacked to one value per byte; the error bound
 * of that header carries over.  What runs: the matrix-core operand B is W - zp_w[n] itself, an int8 in [-15, 15], formed while the
 * nibbles are staged; the epilogue then sees a signed B without a zero point, so the term zp_w' * rowsum(q_x) of the 8-bit route
 * disappears (the quantizing prologue writes no row sums) and what is left is
 *       S = sum_k (q_x - 128 [uint8]) (W - zp_w) - zp_x' * sum_k (W - zp_w)[n],           zp_x' = zp_x - 128 [uint8]
 * in uint32 arithmetic, exact because |S| < 2^31.
 *
 * Launches: those of oq_qdq_function; the column sums (where zp_x' != 0 can be: every unsigned or dynamic X) are one launch that
 * reads the nibbles.
 *
 * Left out, deliberately:
 *   a decode route (M <= 16)      such calls are correct here (the 32-row tile, K split across workgroups) but not tuned.
 *   packed zero points            they stay one value per byte: 1 | N values, nothing to gain.
 *   an odd N                      the rows of a flat-packed [K, N] then start on alternating nibbles: no byte matrix
 *                                 (OQ_ERR_UNSUPPORTED, by name).  Such a tensor is unpacked and goes to oq_qdq_function.
 *   grouped W                     OQ_ERR_UNSUPPORTED, by name: the reference emits none with quantized activations.
 *   fp16 / bf16 X                 OQ_ERR_UNSUPPORTED, by name.
 *   a cache of W's column sums across calls.
 */
#ifndef OQ_HIP_QDQ_FUNCTION_PACKED4_H
#define OQ_HIP_QDQ_FUNCTION_PACKED4_H

#include "oq_hip_qdq_function.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OQ_QDQ_FUNCTION_PACKED4_EXTENSION_VERSION 1

/* OQ_QDQ_FUNCTION_PACKED4_EXTENSION_VERSION of the loaded library */
int32_t oq_qdq_function_packed4_extension_version(void);

/* ---------------------------------------------------------------------------------------------
 *   X, x_mode, x_type, x_scale, x_zero_point, B, b_scale, b_zero_point, out_mode, out_type, out_scale, out_zero_point, Y, stream
 *                as in oq_qdq_function (oq_hip_qdq_function.h).
 *   W            [K, N] values as [K, N / 2] bytes, row-major; `wtype` OQ_UINT4 or OQ_INT4 (oq_qtype; INT4: two's-complement nibbles;
 *                OQ_UINT8 / OQ_INT8 are refused by name: they keep oq_qdq_function); N counts VALUES and is even; leading dimension
 *                ldw >= N / 2 counts BYTES; any byte alignment of the base and of the rows (4-byte aligned rows take dword loads and
 *                give the same bytes).  No byte outside [K, N / 2] is read.
 *   granularity  OQ_TENSOR or OQ_CHANNEL; OQ_GROUP is refused by name.  w_scale (required) fp32; w_zero_point NULL (0), or one value
 *                per byte in the container type (uint8 for OQ_UINT4, int8 for OQ_INT4), inside the 4-bit range, 1 or N of them.
 *   bounds       those of oq_qlinear_matmul (oq_hip_qlinear.h), and K <= 561433 = floor((2^31 - 1) / (255 * 15)): beyond it
 *                |q_x - zp_x| * |W - zp_w| * K can pass 2^31 - 1 and an int32 sum could wrap (the 8-bit entry point stops at 33025).
 *   workspace    256-byte aligned.  oq_qdq_function_packed4_workspace_bytes(M, K, N, x_mode, out_mode) is the sum
 *                Q + R + C + S + P + PX + PO of oq_qdq_function_workspace_bytes, for every K up to this header's bound.  R, the row
 *                sums of q_x, is carved and left unwritten: the two entry points share one layout function, and M * 4 bytes are
 *                not worth a second one.  The query returns 0 (and sets oq_last_error) for a request outside the bounds, with an
 *                unknown mode or with an odd N.
 *   checks       those of oq_qdq_function with the same status codes; a short ldw OQ_ERR_INVALID_ARGUMENT; an odd N, OQ_GROUP, an
 *                fp16 / bf16 X, an 8-bit wtype and K > 561433 OQ_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
size_t oq_qdq_function_packed4_workspace_bytes(int64_t M, int64_t K, int64_t N, int32_t x_mode /* oq_qdq_mode */, int32_t out_mode /* oq_qdq_mode */);
int32_t oq_qdq_function_packed4(const void* X, int32_t atype /* oq_nbits_type */, int64_t M, int64_t K, int64_t lda, int32_t x_mode /* oq_qdq_mode */,
                                int32_t x_type /* oq_ql_type */, const float* x_scale, const void* x_zero_point, const void* W,
                                int32_t wtype /* OQ_UINT4 | OQ_INT4 */, int64_t N, int64_t ldw /* bytes */, int32_t granularity /* oq_strategy */,
                                int64_t group_size, const float* w_scale, const void* w_zero_point, const int32_t* B, const float* b_scale,
                                const int32_t* b_zero_point, int32_t out_mode /* oq_qdq_mode */, int32_t out_type /* oq_ql_type */,
                                const float* out_scale, const void* out_zero_point, float* Y, int64_t ldy, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OQ_HIP_QDQ_FUNCTION_PACKED4_H */
