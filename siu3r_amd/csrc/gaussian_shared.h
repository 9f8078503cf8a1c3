// What the per-Gaussian kernels share: the inclusive scan over a wave and over a workgroup (density.hip's plan, mcmc.hip's scan), and the
// rotation matrix of a raw quaternion (raster.hip, raster_bwd_k3.hip, density.hip's split, mcmc.hip's noise).  Built with -ffp-contract=off,
// the statements of quat_rotation ARE the operation order: the covariance, its backward, the split and the noise agree on R to the bit.
#pragma once
#include "common.h"

// inclusive scan over the wave's 64 lanes
template <typename T>
__device__ inline T wave_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// inclusive scan over a workgroup of NW waves (wave totals through LDS, wsum [NW]); total = the workgroup's sum
template <int NW, typename T>
__device__ inline T block_scan(T v, T* wsum, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_scan(v);
  __syncthreads();  // (the previous round's reads of wsum are over)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  T base = 0, t = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const T s = wsum[w];
    if (w < wave) base += s;
    t += s;
  }
  total = t;
  return v + base;
}

// R(q / |q|), row-major, of a raw quaternion handed over as (w, x, y, z) whatever order the caller stores it in; returns 1 / |q| (the
// covariance backward needs it: its normalised components are the raw ones times this number, as in here)
__device__ inline float quat_rotation(float w, float x, float y, float z, float (&R)[9]) {
  const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
  w *= inv; x *= inv; y *= inv; z *= inv;
  const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0f - 2.0f * (y2 + z2), R[1] = 2.0f * (xy - wz), R[2] = 2.0f * (xz + wy);
  R[3] = 2.0f * (xy + wz), R[4] = 1.0f - 2.0f * (x2 + z2), R[5] = 2.0f * (yz - wx);
  R[6] = 2.0f * (xz - wy), R[7] = 2.0f * (yz + wx), R[8] = 1.0f - 2.0f * (x2 + y2);
  return inv;
}
