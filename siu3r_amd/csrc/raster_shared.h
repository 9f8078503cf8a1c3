// What the composites (raster.hip) and their backward passes (raster_bwd.hip, raster_bwd_k3.hip) must compute identically: a backward
// re-walks the forward's per-pixel transmittance chain and has to stop at the same entry, skip the entries the forward's wave skipped
// (quadrant_mask) and differentiate the projection the forward evaluated (Lens, load_gaussian, project_cov2d), so the translation units
// take these from one place.  Also the frame geometry shared by host and device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int TILE = 16;

// exp(x) for x <= 0 from correctly rounded fp32 operations only (fmaf == v_fma_f32; the same sequence in oracle/raster_ref.c, so
// alpha, the transmittance chain and n_touched are bit-identical on both sides): see exp_det in raster.hip.
// the same value without a branch (the early return becomes a select; x > 0 or NaN: whatever exp_det returns, i.e. the same chain)
__device__ __forceinline__ float exp_det_sel(float x) {
  const float y = x * 1.4426950408889634f;
  const float n = floorf(y + 0.5f);
  const float f = y - n;
  float p = 1.52527338e-5f;
  p = __builtin_fmaf(p, f, 1.54035304e-4f);
  p = __builtin_fmaf(p, f, 1.33335581e-3f);
  p = __builtin_fmaf(p, f, 9.61812911e-3f);
  p = __builtin_fmaf(p, f, 5.55041087e-2f);
  p = __builtin_fmaf(p, f, 2.40226507e-1f);
  p = __builtin_fmaf(p, f, 6.93147181e-1f);
  p = __builtin_fmaf(p, f, 1.0f);
  const float r = ldexpf(p, (int)n);
  return x < -87.0f ? 0.0f : r;
}
// Mahalanobis half-form q = 0.5 (a dx^2 + c dy^2) + b dx dy of a pixel offset, in the shared fused order
__device__ __forceinline__ float conic_sigma(float ca, float cb, float cc, float dx, float dy) {
  const float q = __builtin_fmaf(cc * dy, dy, (ca * dx) * dx);
  return __builtin_fmaf(cb * dx, dy, 0.5f * q);
}
// a c - b^2 of a conic without the cancellation of the naive form (Kahan's 2 x 2 determinant: the rounding error of b * b is recovered with
// one fma; accurate to a few ulps of the RESULT).  The footprint tests that cut lists per quadrant divide by it: for a long thin splat
// seen diagonally a c and b^2 agree to 1e-6 and the naive difference is off by tens of per cent -- a box computed too small would drop
// entries that blend.
__device__ __forceinline__ float conic_det(float a, float b, float c) {
  const float w = b * b;
  const float e = __builtin_fmaf(-b, b, w);
  return __builtin_fmaf(a, c, -w) + e;
}

// Which 8 x 8 quadrants (bit = wave) of the tile at (tile_x0, tile_y0) the alpha >= alpha_min footprint of a staged entry can reach
// (r0 = {mx, my, ..}, r1 = {conic a, b, c, opacity}).  One expression for composite_rgb_kernel and composite_rgb_bwd_kernel: a backward wave
// skips exactly the entries the forward's wave skipped.
// Footprint box: alpha >= alpha_min  =>  sigma <= L = ln(opacity / alpha_min)  =>  |dx| <= sqrt(2 L cov_xx), cov = conic^-1.
// Padded by 1 % + 0.05 px (the exact per-pixel tests of the walk still decide; the box only has to be conservative)
template <bool K3>
__device__ __forceinline__ int quadrant_mask(const float4 r0, const float4 r1, float alpha_min, float tile_x0, float tile_y0) {
  int mk = 15;  // NaN / degenerate conics: no culling, the exact tests decide
  const float L = __logf(r1.w / alpha_min);
  const float det = conic_det(r1.x, r1.y, r1.z);
  if (L <= 0.f) {
    mk = 0;  // opacity below alpha_min: alpha = min(alpha_max, opacity * exp(<= 0)) can never reach it
  } else if (det > 0.f) {
    // (K3: pixel centres sit half a pixel further: the box grows by that much)
    const float ex = sqrtf(2.f * L * r1.z / det) * 1.01f + (K3 ? 0.55f : 0.05f), ey = sqrtf(2.f * L * r1.x / det) * 1.01f + (K3 ? 0.55f : 0.05f);
    const float x0 = r0.x - ex - tile_x0, x1 = r0.x + ex - tile_x0, y0 = r0.y - ey - tile_y0, y1 = r0.y + ey - tile_y0;
    const int cx = (x0 <= 7.f && x1 >= 0.f ? 1 : 0) | (x0 <= 15.f && x1 >= 8.f ? 2 : 0);
    const int cy = (y0 <= 7.f && y1 >= 0.f ? 1 : 0) | (y0 <= 15.f && y1 >= 8.f ? 2 : 0);
    mk = ((cy & 1) ? cx : 0) | ((cy & 2) ? (cx << 2) : 0);
  }
  return mk;
}

// ---- EWA projection of a Gaussian's covariance (project_kernel and both projection backwards) ----------------------------------------
// the per-view lens values of the chain: focal lengths, the limits of the Jacobian clamp on x / z and y / z, the blur added to the diagonal
struct Lens {
  float fx, fy, limx_pos, limx_neg, limy_pos, limy_neg, blur;
};
// mode 0 (3DGS family): the field of view gives the focal lengths, the clamp is symmetric, blur = dilation
__device__ __forceinline__ Lens lens_k2(const siu3r_raster_cam& c) {
  Lens l;
  l.fx = c.width / (2.0f * c.tanfovx);
  l.fy = c.height / (2.0f * c.tanfovy);
  l.limx_pos = l.limx_neg = 1.3f * c.tanfovx;
  l.limy_pos = l.limy_neg = 1.3f * c.tanfovy;
  l.blur = c.dilation;
  return l;
}
// mode 1 (gsplat family): pinhole intrinsics, the clamp follows the principal point, blur = eps2d
__device__ __forceinline__ Lens lens_k3(const siu3r_raster_cam& c) {
  Lens l;
  l.fx = c.fx;
  l.fy = c.fy;
  const float tfx = 0.5f * c.width / l.fx, tfy = 0.5f * c.height / l.fy;
  l.limx_pos = (c.width - c.cx) / l.fx + 0.3f * tfx;
  l.limx_neg = c.cx / l.fx + 0.3f * tfx;
  l.limy_pos = (c.height - c.cy) / l.fy + 0.3f * tfy;
  l.limy_neg = c.cy / l.fy + 0.3f * tfy;
  l.blur = c.eps2d;
  return l;
}

// mean m[3] and the six covariance entries S = (xx, xy, xz, yy, yz, zz) of Gaussian g; cov_stride 6: upper triangle, 9: row-major 3 x 3
__device__ __forceinline__ void load_gaussian(const float* __restrict__ means, const float* __restrict__ cov, int cov_stride, int64_t g, float* m, float* S) {
  m[0] = means[3 * g];
  m[1] = means[3 * g + 1];
  m[2] = means[3 * g + 2];
  const float* cg = cov + (size_t)g * cov_stride;
  const bool tri = cov_stride == 6;
  S[0] = cg[0]; S[1] = cg[1]; S[2] = cg[2]; S[3] = cg[tri ? 3 : 4]; S[4] = cg[tri ? 4 : 5]; S[5] = cg[tri ? 5 : 8];
}

// camera-space point (tx, ty, tz) -> clamped Jacobian J -> M = J W (rows t0, t1; W = world->camera, row-major with stride 4) ->
// 2-D covariance M Sigma M^T + blur I = (c00, c01, c11) and its determinant; everything a backward needs again is kept
struct Cov2D {
  float rz, txz, tyz, cxz, cyz, ctx, cty, j00, j02, j11, j12;
  float t0[3], t1[3], a[3], b[3];  // a = Sigma t0, b = Sigma t1 (Sigma symmetric from the six entries)
  float c00, c01, c11, det;
};
__device__ __forceinline__ Cov2D project_cov2d(const Lens& l, const float* W, float tx, float ty, float tz, const float* S) {
  Cov2D p;
  p.rz = 1.0f / tz;
  p.txz = tx * p.rz, p.tyz = ty * p.rz;
  p.cxz = fminf(l.limx_pos, fmaxf(-l.limx_neg, p.txz)), p.cyz = fminf(l.limy_pos, fmaxf(-l.limy_neg, p.tyz));
  p.ctx = p.cxz * tz, p.cty = p.cyz * tz;
  p.j00 = l.fx * p.rz, p.j02 = -(l.fx * p.ctx) * p.rz * p.rz, p.j11 = l.fy * p.rz, p.j12 = -(l.fy * p.cty) * p.rz * p.rz;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p.t0[i] = p.j00 * W[i] + p.j02 * W[8 + i];
    p.t1[i] = p.j11 * W[4 + i] + p.j12 * W[8 + i];
  }
  const float* t0 = p.t0;
  const float* t1 = p.t1;
  p.a[0] = t0[0] * S[0] + t0[1] * S[1] + t0[2] * S[2], p.a[1] = t0[0] * S[1] + t0[1] * S[3] + t0[2] * S[4], p.a[2] = t0[0] * S[2] + t0[1] * S[4] + t0[2] * S[5];
  p.b[0] = t1[0] * S[0] + t1[1] * S[1] + t1[2] * S[2], p.b[1] = t1[0] * S[1] + t1[1] * S[3] + t1[2] * S[4], p.b[2] = t1[0] * S[2] + t1[1] * S[4] + t1[2] * S[5];
  p.c00 = p.a[0] * t0[0] + p.a[1] * t0[1] + p.a[2] * t0[2] + l.blur;
  p.c01 = p.a[0] * t1[0] + p.a[1] * t1[1] + p.a[2] * t1[2];
  p.c11 = p.b[0] * t1[0] + p.b[1] * t1[1] + p.b[2] * t1[2] + l.blur;
  p.det = p.c00 * p.c11 - p.c01 * p.c01;
  return p;
}

// ---- frame geometry shared by host and device ------------------------------------------------------------------
constexpr int NB_MAX = 1024;            // coarse bins per view (LDS: 40 B per bin in bin_scatter_kernel)
struct Geo {
  int gw, gh, T, cb, nbx, nby, NB;
};
__host__ __device__ inline Geo make_geo(int width, int height) {
  Geo g;
  g.gw = (width + TILE - 1) / TILE;
  g.gh = (height + TILE - 1) / TILE;
  g.T = g.gw * g.gh;
  g.cb = 4;
  for (;;) {
    g.nbx = (g.gw + g.cb - 1) / g.cb;
    g.nby = (g.gh + g.cb - 1) / g.cb;
    g.NB = g.nbx * g.nby;
    if (g.NB <= NB_MAX || g.cb >= 16) break;
    g.cb *= 2;
  }
  return g;
}
// does the packed bin-relative rect cover tile (rtx, rty) of the bin?
__device__ __forceinline__ bool entry_covers(uint32_t pr, int rtx, int rty) {
  const int x0 = pr & 31, y0 = (pr >> 5) & 31, x1 = (pr >> 10) & 31, y1 = (pr >> 15) & 31;
  return rtx >= x0 && rtx < x1 && rty >= y0 && rty < y1;
}

}  // namespace
