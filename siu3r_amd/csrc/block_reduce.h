// What the kernels of splat refinement share: the deterministic reduction over a workgroup of 256 threads (four waves of 64) that the two
// loss kernels use (photo_loss.hip, depth_loss.hip), and the 16-byte alignment test of depth_loss.hip's and gaussian_adam.hip's vector accesses.
#pragma once
#include "common.h"

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

enum class Reduce { Sum, Min, Max };

namespace detail {
template <Reduce OP, typename T>
__device__ inline T combine(T a, T b) {
  return OP == Reduce::Sum ? a + b : (OP == Reduce::Min ? fmin(a, b) : fmax(a, b));
}
}  // namespace detail

// fixed-order reduction of K values per thread: shuffle-down tree per wave, then the four waves in index order through `red` (LDS, [K][4]).
// Every thread returns with the totals in v.  No atomics: two calls give the same bits.
template <Reduce OP, int K, typename T>
__device__ inline void block_reduce(T (&v)[K], T* red /* [K][4] */) {
  using detail::combine;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = combine<OP>(v[k], __shfl_down(v[k], o, 64));
  }
  __syncthreads();  // (the previous use of `red` is over)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[4 * k + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = combine<OP>(combine<OP>(combine<OP>(red[4 * k], red[4 * k + 1]), red[4 * k + 2]), red[4 * k + 3]);
}
