// lanes.h — the cross-lane helpers of the cooperating sinks (device only; glcoop.h with glperm.h, bnquad.h).
#pragma once
#include "field.h"

namespace h2w {

// The cooperating block is ONE wavefront: its LDS operations execute in program order and its lanes run in lockstep, so
// lanes exchange the Poseidon state through LDS with no barrier.  __syncthreads() would also wait for vmcnt(0), i.e. for
// every outstanding record STORE to be acknowledged by memory (~1-2 us) at each of the ~90 exchange points of a
// permutation; this waits for LDS only.
__device__ __forceinline__ void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int src) {      // src: wave-uniform
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
template <int N> __device__ __forceinline__ uint64_t row_shr64(uint64_t v) {      // lane i <- lane i - N of its 16-lane row, 0 where there is none
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, 0x110 + N, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), 0x110 + N, 0xf, 0xf, true);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace h2w
