// The transposing butterfly of the decode routes (matmul_nbits_decode.hip: fp32 sums over 32 or 64 lanes; qlinear_decode.hip:
// uint32 sums over a wave): a fixed order, log2(LK) additions per value, about one shuffle per value.
#pragma once

#include "oq_common.hpp"

namespace oq {
namespace {

// CNT values per lane (a power of two, at most LK), LK lanes: the sum over the lanes of value (c mod the original CNT) ends in v[0]
// of lane c.  Called with OFF = 1.
template <int CNT, int OFF, int LK, typename T>
__device__ __forceinline__ void lanes_reduce(T* v, int c) {
    if constexpr (OFF < LK) {
        if constexpr (CNT > 1) {
            const bool up = (c & OFF) != 0;
#pragma unroll
            for (int i = 0; i < CNT / 2; ++i) {
                const T keep = up ? v[2 * i + 1] : v[2 * i], send = up ? v[2 * i] : v[2 * i + 1];
                v[i] = keep + __shfl_xor(send, OFF, kWave);
            }
            lanes_reduce<CNT / 2, OFF * 2, LK>(v, c);
        } else {
            v[0] += __shfl_xor(v[0], OFF, kWave);
            lanes_reduce<1, OFF * 2, LK>(v, c);
        }
    }
}

}  // namespace
}  // namespace oq
