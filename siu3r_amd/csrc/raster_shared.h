// What the composites (raster.hip) and their backward passes (raster_bwd.hip, raster_bwd_k3.hip) must compute identically: a backward
// re-walks the forward's per-pixel transmittance chain and has to stop at the same entry, so the translation units take these from one place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
