// Host-side declarations shared by the RTN sources (rtn.hip, rtn_resident.hip, rtn_mse.hip, rtn_half.hip) and their callers inside the
// library (awq.hip, gptq_loop.hip).  Not part of the C ABI.
#pragma once

#include <atomic>

#include "oq_common.hpp"

namespace oq {

struct RtnPtrs;   // rtn.hip: the device view of oq_rtn_ptrs

// One RTN call: the arguments of oq_rtn_quantize_f32 plus what only some entry points pass.  Every input that decides which
// kernel runs is a field here.
struct RtnCall {
    const float* W;
    int64_t K, N, ldw;
    int32_t qtype, strategy;
    int64_t group_size;
    int32_t symmetric, reduce_range;
    float clip_ratio;
    int32_t mse;
    void* q;           // may be null with emit_q == false (parameters only)
    float* scale;
    void* zp;
    int32_t layout;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    bool emit_q = true;
    // oq_rtn_quantize_batched_f32 / _ptrs_f32: `batch` matrices in one launch of the group kernels, matrix b at W + b * w_stride
    // (fp32 elements) and q + b * q_stride (bytes), or at table[b] (device memory) when a table is given
    int64_t batch = 1, w_stride = 0, q_stride = 0;
    const RtnPtrs* table = nullptr;
    // oq_rtn_quantize_stateful_f32: the caller's zeroed, self-cleaning state
    void* state = nullptr;
    size_t state_bytes = 0;
};

// rtn.hip
int32_t rtn_impl(const RtnCall& c);
// rows per (scale, zp) of a strategy: utils.py:16-22 for groups, K for channel / tensor; refuses a bad group_size or strategy
int32_t resolve_group(int32_t strategy, int64_t K, int64_t group_size, int64_t* g);
// matrices of one shape that share a launch of a pointer-table entry point (oq_rtn_quantize_ptrs_f32 / _h16): a parameter budget
// per launch, capped by blockIdx.y
int64_t matrices_per_launch(int64_t K, int64_t N, int64_t count);
// pass 3 of the three-launch path, also the final pass of the MSE search: K1 with stored parameters
int32_t launch_quantize_kn(const float* W, int64_t K, int64_t N, int64_t ldw, int64_t g, int64_t kgroups, const float* scale,
                           const uint8_t* zp, uint8_t* q, const QGrid& grid, int32_t zp_signed, bool tensor, hipStream_t s,
                           int32_t layout);

// rtn_mse.hip
int32_t rtn_mse_impl(const float* W, int64_t K, int64_t N, int64_t ldw, const QGrid& grid, int32_t strategy,
                     int64_t g, void* q_out, float* scale_out, void* zp_out, int32_t zp_signed, void* workspace,
                     size_t workspace_bytes, hipStream_t s, bool emit_q);
size_t rtn_mse_workspace(int64_t K, int64_t N, int32_t strategy, int64_t g);
// the same search on a 2-byte matrix (`wtype`: an oq_wtype); q_out null: parameters only.  The caller (oq_rtn_mse_h16) has made every check.
int32_t rtn_mse_half_impl(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, const QGrid& grid, int32_t strategy, int64_t g,
                          void* q_out, float* scale_out, void* zp_out, void* workspace, size_t workspace_bytes, hipStream_t s);

// rtn_half.hip: the stored-parameter pass of the two-launch route (half_quantize: [K, N] bytes, the IEEE division), also the final
// pass of the half MSE search; parameter col * kgroups + kg, or the one pair of a tensor
int32_t launch_half_quantize_kn(const void* W, int32_t wtype, int64_t K, int64_t N, int64_t ldw, int64_t g, int64_t kgroups, float* scale,
                                uint8_t* zp, uint8_t* q, const QGrid& grid, bool tensor, hipStream_t s);

// rtn_resident.hip: the one-read channel / tensor / tall-group kernels ("ticketed": their workgroups wait for one another)
bool rtn_resident_eligible(int64_t K, int64_t N, int64_t ldw, const float* W, const void* q, int32_t strategy, int64_t g, int32_t layout,
                           bool emit_q, size_t workspace_bytes);
int32_t rtn_resident_impl(const float* W, int64_t K, int64_t N, int64_t ldw, const QGrid& grid, int32_t strategy, int64_t g, uint8_t* q,
                          float* scale, uint8_t* zp, int32_t layout, void* workspace, size_t workspace_bytes, hipStream_t s, bool zeroed_state);
size_t rtn_resident_workspace(int64_t K, int64_t N, int32_t strategy, int64_t g);
bool rtn_stream_is_capturing(hipStream_t s);
// A launch whose workgroups wait for others of the same launch goes between these two: launches of one device are chained
// (rtn_resident.hip::TicketChain).  A failing begin holds nothing.
int32_t ticket_chain_begin(hipStream_t s);
void ticket_chain_end(hipStream_t s);
// Workgroups of `kernel` (`threads` per block, `dynamic_lds` bytes of dynamic LDS) that the current device runs at once: CUs x the
// occupancy query.  `cache` is the caller's, one per kernel, indexed by device: the first answer is kept (the query costs
// microseconds, small calls are host-bound).  0 when the query fails.
int resident_slots(std::atomic<int> (&cache)[64], const void* kernel, int threads, size_t dynamic_lds = 0);

}  // namespace oq
