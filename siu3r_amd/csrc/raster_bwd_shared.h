// What the two rasterizer backward units (raster_bwd.hip: the 3DGS family, raster_bwd_k3.hip: the gsplat family) share: the layout of
// the per-(view, Gaussian) screen-space gradient record, the wave sum and the SH basis with its direction gradient.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// per-(view, Gaussian) gradient record written by the composite backward
enum { GR_MX = 0, GR_MY, GR_CA, GR_CB, GR_CC, GR_OP, GR_R, GR_G, GR_B, GR_Z, GR_N };

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
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

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace
