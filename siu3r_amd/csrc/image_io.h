// How the streaming kernels of the cameras' colour models (camera.hip, bilagrid.hip) read and write images: PX consecutive pixels of a view's
// three channels per thread, as stored.  The strided side (`in`, g_in) goes through four element strides held by the kernel's argument
// struct `a` (a.s[4] = view, channel, row, column; a.W; a.P = H * W; a.layout); the contiguous side (out, g_out) is [3][P] planes.  16-byte
// accesses where the layout is dense planes or dense pixels on 16-byte aligned bases, scalar accesses otherwise.
#pragma once
#include "block_reduce.h"

constexpr int PX = 4;  // consecutive pixels per thread and round

enum Layout { PLANES = 0, PIXELS = 1, STRIDED = 2 };  // dense [3][H*W] / dense [H*W][3] / anything the four strides express

// PX consecutive pixels of the three channels of one view, stored as `layout` says; 0 past the end of the view
template <class A>
__device__ inline void load3(const float* base, const A& a, int i0, bool vec, float (&x)[3][PX]) {
  if (vec && i0 + PX <= a.P) {
    if (a.layout == PLANES) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 q = *reinterpret_cast<const float4*>(base + c * a.s[1] + i0);
        x[c][0] = q.x, x[c][1] = q.y, x[c][2] = q.z, x[c][3] = q.w;
      }
    } else {  // PIXELS: 12 consecutive floats
      const float4* q = reinterpret_cast<const float4*>(base + (int64_t)i0 * 3);
      const float4 q0 = q[0], q1 = q[1], q2 = q[2];
      x[0][0] = q0.x, x[1][0] = q0.y, x[2][0] = q0.z, x[0][1] = q0.w;
      x[1][1] = q1.x, x[2][1] = q1.y, x[0][2] = q1.z, x[1][2] = q1.w;
      x[2][2] = q2.x, x[0][3] = q2.y, x[1][3] = q2.z, x[2][3] = q2.w;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = i0 + k;
    const bool in = i < a.P;
    const int y = in ? i / a.W : 0, xx = in ? i - y * a.W : 0;
    const float* p = base + y * a.s[2] + xx * a.s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c][k] = in ? p[c * a.s[1]] : 0.f;
  }
}

template <class A>
__device__ inline void store3(float* base, const A& a, int i0, bool vec, const float (&x)[3][PX]) {
  if (vec && i0 + PX <= a.P) {
    if (a.layout == PLANES) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(base + c * a.s[1] + i0) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
    } else {
      float4* q = reinterpret_cast<float4*>(base + (int64_t)i0 * 3);
      q[0] = make_float4(x[0][0], x[1][0], x[2][0], x[0][1]);
      q[1] = make_float4(x[1][1], x[2][1], x[0][2], x[1][2]);
      q[2] = make_float4(x[2][2], x[0][3], x[1][3], x[2][3]);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = i0 + k;
    if (i < a.P) {
      const int y = i / a.W, xx = i - y * a.W;
      float* p = base + y * a.s[2] + xx * a.s[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c * a.s[1]] = x[c][k];
    }
  }
}

// the contiguous [3][P] planes of out / g_out
__device__ inline void load_planes(const float* base, int P, int i0, bool vec, float (&x)[3][PX]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pl = base + (int64_t)c * P;
    if (vec && i0 + PX <= P) {
      const float4 q = *reinterpret_cast<const float4*>(pl + i0);
      x[c][0] = q.x, x[c][1] = q.y, x[c][2] = q.z, x[c][3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k) x[c][k] = i0 + k < P ? pl[i0 + k] : 0.f;
    }
  }
}

__device__ inline void store_planes(float* base, int P, int i0, bool vec, const float (&x)[3][PX]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* pl = base + (int64_t)c * P;
    if (vec && i0 + PX <= P) {
      *reinterpret_cast<float4*>(pl + i0) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k)
        if (i0 + k < P) pl[i0 + k] = x[c][k];
    }
  }
}

// one decision per workgroup: a thread's pixels start a multiple of 16 bytes (PLANES) or 48 bytes (PIXELS) into the view, so only the bases matter
template <class A>
__device__ inline bool strided_vec(const float* base, const A& a) {
  if (a.layout == PLANES) return aligned16(base) && aligned16(base + a.s[1]) && aligned16(base + 2 * a.s[1]);
  return a.layout == PIXELS && aligned16(base);
}
__device__ inline bool planes_vec(const float* base, int P) { return aligned16(base) && aligned16(base + P) && aligned16(base + 2 * (int64_t)P); }
