// What the two rasterizer backward units (raster_bwd.hip: the 3DGS family, raster_bwd_k3.hip: the gsplat family) share: the layout of
// the per-(view, Gaussian) screen-space gradient record, the wave sum and the per-workgroup partial rows with their reduction, the
// backward of the covariance projection (project_cov2d, raster_shared.h), the SH basis with its direction gradient and the SH colour
// backward, and the host-side check of a call's views.
#pragma once
#include <hip/hip_runtime.h>

#include "raster_shared.h"

namespace {

// per-(view, Gaussian) gradient record written by the composite backward
enum { GR_MX = 0, GR_MY, GR_CA, GR_CB, GR_CC, GR_OP, GR_R, GR_G, GR_B, GR_Z, GR_N };

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// Sum of N per-thread terms over the workgroup (256 threads) into row[0 .. N), fixed order: wave sums, then the four waves through
// LDS; row[N .. OUT) = 0.  Every thread of the workgroup must call it (barriers); it may be called again at once.
template <int N, int OUT = N>
__device__ __forceinline__ void block_sum_row(const float* x, float* __restrict__ row) {
  __shared__ float s[4][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float t = wave_sum(x[k]);
    if (lane == 0) s[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < OUT) {
    const int k = threadIdx.x;
    row[k] = k < N ? s[0][k] + s[1][k] + s[2][k] + s[3][k] : 0.f;
  }
  __syncthreads();
}

// part [nblk, V, N] (the partial rows of the projection backwards) -> out [V, OUT]: one workgroup per view, entries past N are 0
// (N = 6, OUT = 6: the se(3) pose gradient; N = 12, OUT = 16: d loss / d [R | t] as a 4 x 4 matrix with a zero fourth row)
template <int N, int OUT>
__global__ __launch_bounds__(256) void rows_reduce_kernel(int V, int64_t nblk, const float* __restrict__ part, float* __restrict__ out) {
  const int v = blockIdx.x;
  float acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = 0.f;
  for (int64_t b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] += part[(b * V + v) * N + k];
  block_sum_row<N, OUT>(acc, out + v * OUT);
}

// ---- projection backward: what both camera modes share -------------------------------------------------------------------------------
// d loss / d conic (gca, gcb, gcc) -> through the conic inverse and the 2-D covariance M Sigma M^T (p: the forward chain, project_cov2d)
// to the rows of M (dt0, dt1), the Jacobian entries (dj..) and, added into gS[6], the Gaussian's covariance.
// DIRECT (compile time): e00, e01, e11 = d loss / d (c00, c01, c11) that reaches the 2-D covariance NOT through the conic (the anti-aliased
// projection's opacity compensation; c01 counted once, as d01 is) are added to the conic's contribution before the chain, so that one chain
// carries both.  Without it the three arguments are not read and the code is the one it was.
struct Cov2DGrad {
  float dt0[3], dt1[3], dj00, dj02, dj11, dj12;
};
template <bool DIRECT = false>
__device__ __forceinline__ Cov2DGrad project_cov2d_bwd(const Cov2D& p, const float* W, float gca, float gcb, float gcc, float* gS, float e00 = 0.f,
                                                       float e01 = 0.f, float e11 = 0.f) {
  const float* t0 = p.t0;
  const float* t1 = p.t1;
  const float rdet = 1.0f / p.det;
  const float ca = p.c11 * rdet, cb = -p.c01 * rdet, cc = p.c00 * rdet;
  // conic inverse
  const float dLddet = -(gca * ca + gcb * cb + gcc * cc) * rdet;
  float d00 = gcc * rdet + dLddet * p.c11, d11 = gca * rdet + dLddet * p.c00, d01 = -gcb * rdet - 2.0f * dLddet * p.c01;
  if constexpr (DIRECT) {
    d00 += e00;
    d01 += e01;
    d11 += e11;
  }
  // 2-D covariance = M Sigma M^T (+ blur), M = J W (rows t0, t1)
  Cov2DGrad q;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    q.dt0[i] = 2.0f * d00 * p.a[i] + d01 * p.b[i];
    q.dt1[i] = 2.0f * d11 * p.b[i] + d01 * p.a[i];
  }
  gS[0] += d00 * t0[0] * t0[0] + d01 * t0[0] * t1[0] + d11 * t1[0] * t1[0];
  gS[3] += d00 * t0[1] * t0[1] + d01 * t0[1] * t1[1] + d11 * t1[1] * t1[1];
  gS[5] += d00 * t0[2] * t0[2] + d01 * t0[2] * t1[2] + d11 * t1[2] * t1[2];
  gS[1] += 2.0f * d00 * t0[0] * t0[1] + d01 * (t0[0] * t1[1] + t0[1] * t1[0]) + 2.0f * d11 * t1[0] * t1[1];
  gS[2] += 2.0f * d00 * t0[0] * t0[2] + d01 * (t0[0] * t1[2] + t0[2] * t1[0]) + 2.0f * d11 * t1[0] * t1[2];
  gS[4] += 2.0f * d00 * t0[1] * t0[2] + d01 * (t0[1] * t1[2] + t0[2] * t1[1]) + 2.0f * d11 * t1[1] * t1[2];
  q.dj00 = q.dt0[0] * W[0] + q.dt0[1] * W[1] + q.dt0[2] * W[2], q.dj02 = q.dt0[0] * W[8] + q.dt0[1] * W[9] + q.dt0[2] * W[10];
  q.dj11 = q.dt1[0] * W[4] + q.dt1[1] * W[5] + q.dt1[2] * W[6], q.dj12 = q.dt1[0] * W[8] + q.dt1[1] * W[9] + q.dt1[2] * W[10];
  return q;
}

// every view of a call: camera mode `mode`, one frame size
inline int check_views(const siu3r_raster_cam* cams, int V, int mode, const char* who) {
  SIU3R_CHECK(cams && V >= 1 && V <= 65535, "%s: bad view array (V = %d)", who, V);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK(cams[v].mode == mode && cams[v].width == cams[0].width && cams[v].height == cams[0].height && cams[v].width > 0 && cams[v].height > 0,
                "%s: the backward covers the %s family (mode %d) with one frame size per call", who, mode == 0 ? "3DGS" : "gsplat", mode);
  return 0;
}

// ---- SH basis with its gradient w.r.t. the (unit) view direction ---------------------------------------------------------------------
struct Dual {  // value + d/dx, d/dy, d/dz
  float v, x, y, z;
};
__device__ __forceinline__ Dual dconst(float c) { return {c, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Dual operator-(Dual a, float b) { return {a.v - b, a.x, a.y, a.z}; }
__device__ __forceinline__ Dual operator+(Dual a, float b) { return {a.v + b, a.x, a.y, a.z}; }
__device__ __forceinline__ Dual operator*(float s, Dual a) { return {s * a.v, s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.x * b.v + a.v * b.x, a.y * b.v + a.v * b.y, a.z * b.v + a.v * b.z}; }

__constant__ float c_B2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
__constant__ float c_B3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
__constant__ float c_B4[9] = {2.5033429417967046f, -1.7701307697799304f, 0.9461746957575601f, -0.6690465435572892f, 0.10578554691520431f, -0.6690465435572892f, 0.47308734787878004f, -1.7701307697799304f, 0.6258357354491761f};

// calls f(k, basis_k) for the coefficients the forward's polynomial uses (project_kernel: degree deg, band 4 only with band4); k is a
// compile-time constant at every call site
template <class F>
__device__ __forceinline__ void sh_basis(float dx_, float dy_, float dz_, int deg, bool band4, F&& f) {
  const Dual x = {dx_, 1.f, 0.f, 0.f}, y = {dy_, 0.f, 1.f, 0.f}, z = {dz_, 0.f, 0.f, 1.f};
  f(0, dconst(0.28209479177387814f));
  if (deg < 1) return;
  const float C1 = 0.4886025119029199f;
  f(1, -C1 * y);
  f(2, C1 * z);
  f(3, -C1 * x);
  if (deg < 2) return;
  const Dual xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  f(4, c_B2[0] * xy);
  f(5, c_B2[1] * yz);
  f(6, c_B2[2] * (2.0f * zz - xx - yy));
  f(7, c_B2[3] * xz);
  f(8, c_B2[4] * (xx - yy));
  if (deg < 3) return;
  f(9, c_B3[0] * (y * (3.0f * xx - yy)));
  f(10, c_B3[1] * (xy * z));
  f(11, c_B3[2] * (y * (4.0f * zz - xx - yy)));
  f(12, c_B3[3] * (z * (2.0f * zz - 3.0f * xx - 3.0f * yy)));
  f(13, c_B3[4] * (x * (4.0f * zz - xx - yy)));
  f(14, c_B3[5] * (z * (xx - yy)));
  f(15, c_B3[6] * (x * (xx - 3.0f * yy)));
  if (deg < 4 || !band4) return;
  f(16, c_B4[0] * (xy * (xx - yy)));
  f(17, c_B4[1] * (yz * (3.0f * xx - yy)));
  f(18, c_B4[2] * (xy * (7.0f * zz - 1.0f)));
  f(19, c_B4[3] * (yz * (7.0f * zz - 3.0f)));
  f(20, c_B4[4] * (zz * (35.0f * zz - 30.0f) + 3.0f));
  f(21, c_B4[5] * (xz * (7.0f * zz - 3.0f)));
  f(22, c_B4[6] * ((xx - yy) * (7.0f * zz - 1.0f)));
  f(23, c_B4[7] * (xz * (xx - 3.0f * yy)));
  f(24, c_B4[8] * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy)));
}

// unit view direction d = (m - campos) / |m - campos| with 1 / |m - campos|
struct ViewDir {
  float x, y, z, inv;
};
__device__ __forceinline__ ViewDir view_dir(const float* m, const float* campos) {
  const float ddx = m[0] - campos[0], ddy = m[1] - campos[1], ddz = m[2] - campos[2];
  const float len = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz), inv = 1.0f / len;
  return {ddx * inv, ddy * inv, ddz * inv, inv};
}
// Backward of rgb = max(sum_k B_k(d) coef(k, ch) + 0.5, 0) for the upstream colour gradient gcol[3]: a channel clamped at 0 passes
// nothing; sink(k, ch, value) takes d loss / d coef(k, ch) for the coefficients the forward's polynomial uses.  Returns d loss / d m
// through the direction: the gradient w.r.t. d, projected off d and divided by the length.
template <class Coef, class Sink>
__device__ __forceinline__ float3 sh_color_bwd(const ViewDir d, int deg, bool band4, const float* gcol, Coef&& coef, Sink&& sink) {
  // which channels the +0.5 / clamp-at-0 left alive
  float rsum[3] = {0.5f, 0.5f, 0.5f};
  sh_basis(d.x, d.y, d.z, deg, band4, [&](int k, Dual bk) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rsum[ch] += bk.v * coef(k, ch);
  });
  float gl[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) gl[ch] = rsum[ch] < 0.0f ? 0.0f : gcol[ch];
  float gd[3] = {0.f, 0.f, 0.f};
  sh_basis(d.x, d.y, d.z, deg, band4, [&](int k, Dual bk) {
    float s = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      sink(k, ch, bk.v * gl[ch]);
      s += gl[ch] * coef(k, ch);
    }
    gd[0] += s * bk.x;
    gd[1] += s * bk.y;
    gd[2] += s * bk.z;
  });
  const float dd = gd[0] * d.x + gd[1] * d.y + gd[2] * d.z;
  return make_float3((gd[0] - d.x * dd) * d.inv, (gd[1] - d.y * dd) * d.inv, (gd[2] - d.z * dd) * d.inv);
}

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace
