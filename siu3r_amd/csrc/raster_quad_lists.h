// The per-8 x 8-quadrant lists of the N-channel composite, shared by its forward (raster.hip) and its backward (raster_bwd_k3.hip) only:
// the two units that walk them.  Include after common.h and raster_shared.h.
#pragma once
#include "raster_shared.h"

namespace {

// ---- per-8 x 8-quadrant lists of the N-channel composite (composite_feat5_kernel) and of its backward -------------------------------
// The lists are cut per quadrant by a conservative extent test, order kept (4 B per (quadrant, entry) pair): an entry dropped here can
// never pass a pixel's test, so a walk over the quadrant list is the walk over the tile list.
__global__ __launch_bounds__(256) void ql_build_kernel(const siu3r_raster_cam* __restrict__ cams, Geo geo, const int32_t* __restrict__ tile_start,
                                                       const int32_t* __restrict__ ids, int64_t cap_d, const float* __restrict__ rec, int64_t G,
                                                       int32_t* __restrict__ qids, int32_t* __restrict__ qcnt) {
  __shared__ int s_w[4][4];  // [quadrant][wave] survivors of the current slice
  const int v = blockIdx.y, tile = blockIdx.x, tx = tile % geo.gw, ty = tile / geo.gw;
  const siu3r_raster_cam& c = cams[v];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* ts = tile_start + (int64_t)v * (geo.T + 2);
  const int32_t* idp = ids + (int64_t)v * cap_d;
  const int beg = ts[tile], end = ts[tile + 1], len = end - beg;
  int32_t* qo = qids + (int64_t)v * 4 * cap_d + 4 * (int64_t)beg;
  const float alpha_min = c.alpha_min;
  const float tx0 = (float)(tx * TILE), ty0 = (float)(ty * TILE);
  int run[4] = {0, 0, 0, 0};
  for (int b = beg; b < end; b += 256) {
    const int i = b + threadIdx.x;
    unsigned bits = 0;
    int id = 0;
    if (i < end) {
      id = idp[i];
      const float4* rp = (const float4*)(rec + 12 * ((int64_t)v * G + id));
      const float4 r0 = rp[0], r1 = rp[1];
      // alpha >= alpha_min  <=>  sigma <= L = ln(opacity / alpha_min); on that ellipse |dx| <= sqrt(2 L c / det), |dy| <= sqrt(2 L a / det).
      // Conservative (margins far above the rounding of exp_det and of this bound): an entry dropped here can never pass the per-pixel
      // test of the composite, an entry kept needlessly only costs time.
      const float det = conic_det(r1.x, r1.y, r1.z);
      const float L = logf(r1.w / alpha_min) * 1.001f + 0.001f;
      bits = 0xfu;
      if (L < 0.f) bits = 0;
      else if (det > 0.f && L == L) {
        const float ex = sqrtf(2.0f * L * r1.z / det) + 0.01f, ey = sqrtf(2.0f * L * r1.x / det) + 0.01f;
        if (ex == ex && ey == ey) {
          const bool xl = r0.x - ex <= tx0 + 7.5f && r0.x + ex >= tx0 + 0.5f, xr = r0.x - ex <= tx0 + 15.5f && r0.x + ex >= tx0 + 8.5f;
          const bool yt = r0.y - ey <= ty0 + 7.5f && r0.y + ey >= ty0 + 0.5f, yb = r0.y - ey <= ty0 + 15.5f && r0.y + ey >= ty0 + 8.5f;
          bits = (xl && yt ? 1u : 0u) | (xr && yt ? 2u : 0u) | (xl && yb ? 4u : 0u) | (xr && yb ? 8u : 0u);
        }
      }
    }
    unsigned long long m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      m[q] = __ballot((bits >> q) & 1u);
      if (lane == 0) s_w[q][wave] = __popcll(m[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int off = run[q] + __popcll(m[q] & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) off += s_w[q][w];
      if ((bits >> q) & 1u) qo[(int64_t)q * len + off] = id;
      run[q] += s_w[q][0] + s_w[q][1] + s_w[q][2] + s_w[q][3];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) qcnt[((int64_t)v * geo.T + tile) * 4 + threadIdx.x] = run[threadIdx.x];
}

}  // namespace
