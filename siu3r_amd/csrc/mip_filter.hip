// The 3-D smoothing filter of Mip-Splatting (Yu et al. 2024) for gfx950: every Gaussian's size is bounded below by the sampling rate of the
// training cameras, so that a refined set stays right when it is rendered at another resolution or distance.
//
//   siu3r_mip_filter3d   filter [G] from the means and the training cameras.  Three launches on the stream:
//                        cameras    one thread per view: world->camera rows [R | t] = inverse of the camera-to-world matrix (fp64, rounded
//                                   once; its fourth row is taken as (0, 0, 0, 1)) and fx, fy, cx, cy = Kn * (W, H) into the workspace
//                        depth      one thread per Gaussian, looping over the views: d = the smallest camera-space z over the views that
//                                   SEE it (z > z_near and the pinhole pixel fx x / z + cx, fy y / z + cy inside the frame grown by
//                                   `margin` on every side), 0 when no view does; the largest d goes to one workspace word as a maximum of
//                                   bit patterns (positive floats order like their bits): order-independent, so the result is reproducible
//                        finish     filter = (sqrt(variance) * d) / focal, an unseen Gaussian taking the largest d of the seen ones
//                                   (Mip-Splatting's rule); focal = the largest fx over the views.  Nothing seen at all: all zeros.
//                        The principal point comes from Kn.  Mip-Splatting itself assumes the image centre (it tests the NDC-like
//                        coordinates x / z * focal + W / 2); with cx = W / 2, cy = H / 2 the two tests are the same.
//   siu3r_mip_apply      scales_f = sqrt(s^2 + f^2), opac_f = o * prod_i q_i with q_i = |s_i| / scales_f_i (= sqrt(s_i^2 / (s_i^2 + f^2)):
//                        the ratio is formed per axis, so neither prod s_i^2 nor prod (s_i^2 + f^2) is ever formed and nothing overflows
//                        or flushes to zero that the result does not).  An axis with s_i = f = 0 has q_i = 1.
//   siu3r_mip_apply_bwd  g_scales_i = g_scales_f_i s_i / scales_f_i + g_opac_f o (prod_{j != i} q_j) sign(s_i) (f / scales_f_i)^2 / scales_f_i,
//                        g_opac = g_opac_f prod q.  The filter gets no gradient.
//
// All three are streaming kernels, one record per lane, no scratch.  The [G,3] arrays travel through LDS: a workgroup's 256 rows are 768
// consecutive floats, loaded / stored as three fully coalesced rounds and read / written per lane at a stride of three words (odd: no bank
// conflict).  Built like the rest of the library with -ffp-contract=off and -fno-slp-vectorize.
#include "common.h"

namespace {

constexpr int MIP_WS_CAM = 16;  // floats per view in the workspace: R row 0, t0, R row 1, t1, R row 2, t2, fx, fy, cx, cy

// a workgroup's 256 rows of a [G,3] array: global -> LDS (768 floats), coalesced; zeros past the end
__device__ __forceinline__ void rows3_load(const float* __restrict__ src, int64_t G, float* lds) {
  const int64_t base = (int64_t)blockIdx.x * 768, end = G * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = k * 256 + threadIdx.x;
    lds[i] = base + i < end ? src[base + i] : 0.f;
  }
  __syncthreads();
}
// LDS (768 floats) -> a workgroup's 256 rows of a [G,3] array, coalesced
__device__ __forceinline__ void rows3_store(float* __restrict__ dst, int64_t G, const float* lds) {
  const int64_t base = (int64_t)blockIdx.x * 768, end = G * 3;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = k * 256 + threadIdx.x;
    if (base + i < end) dst[base + i] = lds[i];
  }
}

__global__ void mip_cams_kernel(int V, int width, int height, const float* __restrict__ c2w, const float* __restrict__ Kn, float* __restrict__ ws) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const float* E = c2w + 16 * v;
  const double a = E[0], b = E[1], c = E[2], d = E[4], e = E[5], f = E[6], g = E[8], h = E[9], k = E[10];
  const double t[3] = {(double)E[3], (double)E[7], (double)E[11]};
  const double det = a * (e * k - f * h) - b * (d * k - f * g) + c * (d * h - e * g), rd = 1.0 / det;  // (singular: inf / NaN rows, nothing is seen)
  const double Ri[9] = {(e * k - f * h) * rd, (c * h - b * k) * rd, (b * f - c * e) * rd, (f * g - d * k) * rd, (a * k - c * g) * rd,
                        (c * d - a * f) * rd, (d * h - e * g) * rd, (b * g - a * h) * rd, (a * e - b * d) * rd};
  float* o = ws + MIP_WS_CAM * v;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    o[4 * r] = (float)Ri[3 * r];
    o[4 * r + 1] = (float)Ri[3 * r + 1];
    o[4 * r + 2] = (float)Ri[3 * r + 2];
    o[4 * r + 3] = (float)-(Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1] + Ri[3 * r + 2] * t[2]);
  }
  const float* K = Kn + 9 * v;
  o[12] = K[0] * (float)width;
  o[13] = K[4] * (float)height;
  o[14] = K[2] * (float)width;
  o[15] = K[5] * (float)height;
}

__global__ __launch_bounds__(256) void mip_depth_kernel(int V, int width, int height, int64_t G, const float* __restrict__ means, float z_near, float margin,
                                                        const float* __restrict__ ws, float* __restrict__ filter, unsigned int* __restrict__ dmax) {
  __shared__ float s_m[768];
  rows3_load(means, G, s_m);
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float m0 = s_m[3 * threadIdx.x], m1 = s_m[3 * threadIdx.x + 1], m2 = s_m[3 * threadIdx.x + 2];
  const float x_lo = -margin * (float)width, x_hi = (1.0f + margin) * (float)width, y_lo = -margin * (float)height, y_hi = (1.0f + margin) * (float)height;
  float d = 0.f;  // 0: no view sees it (a seen depth is > z_near >= 0)
  for (int v = 0; v < V; ++v) {
    const float* c = ws + MIP_WS_CAM * v;  // (uniform address: scalar loads)
    const float x = c[0] * m0 + c[1] * m1 + c[2] * m2 + c[3];
    const float y = c[4] * m0 + c[5] * m1 + c[6] * m2 + c[7];
    const float z = c[8] * m0 + c[9] * m1 + c[10] * m2 + c[11];
    const float px = c[12] * x / z + c[14], py = c[13] * y / z + c[15];
    // (a NaN mean fails every comparison: unseen)
    const bool seen = z > z_near && px >= x_lo && px <= x_hi && py >= y_lo && py <= y_hi;
    if (seen) d = d > 0.f ? fminf(d, z) : z;
  }
  if (gi >= G) d = 0.f;
  if (gi < G) filter[gi] = d;
  // the largest seen depth: positive floats order like their bit patterns -> a wave maximum, then one integer atomic per wave
  unsigned int u = __float_as_uint(d);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u = max(u, (unsigned int)__shfl_xor((int)u, o));
  if ((threadIdx.x & 63) == 0 && u) atomicMax(dmax, u);
}

__global__ __launch_bounds__(256) void mip_finish_kernel(int V, int64_t G, float variance, const float* __restrict__ ws, const unsigned int* __restrict__ dmax,
                                                         float* __restrict__ filter) {
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gi >= G) return;
  float focal = ws[12];
  for (int v = 1; v < V; ++v) focal = fmaxf(focal, ws[MIP_WS_CAM * v + 12]);
  const float far_d = __uint_as_float(*dmax);
  float d = filter[gi];
  if (!(d > 0.f)) d = far_d;
  filter[gi] = far_d > 0.f ? (sqrtf(variance) * d) / focal : 0.f;
}

// sf_i = sqrt(s_i^2 + f^2), q_i = |s_i| / sf_i (1 where sf_i = 0)
__device__ __forceinline__ void mip_axes(const float* s, float f, float* sf, float* q) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sf[i] = sqrtf(s[i] * s[i] + f * f);
    q[i] = sf[i] > 0.f ? fabsf(s[i]) / sf[i] : 1.0f;
  }
}

__global__ __launch_bounds__(256) void mip_apply_kernel(int64_t G, const float* __restrict__ scales, const float* __restrict__ opac, const float* __restrict__ filter,
                                                        float* __restrict__ scales_f, float* __restrict__ opac_f) {
  __shared__ float s_s[768];
  rows3_load(scales, G, s_s);
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = gi < G;
  const float s[3] = {s_s[3 * threadIdx.x], s_s[3 * threadIdx.x + 1], s_s[3 * threadIdx.x + 2]};
  const float f = live ? filter[gi] : 0.f;
  float sf[3], q[3];
  mip_axes(s, f, sf, q);
  if (live) opac_f[gi] = opac[gi] * ((q[0] * q[1]) * q[2]);
  // (every lane has read its own three words above and writes only those: no barrier is needed in between; rows3_store has the one in
  // front of the coalesced reads)
#pragma unroll
  for (int i = 0; i < 3; ++i) s_s[3 * threadIdx.x + i] = sf[i];
  rows3_store(scales_f, G, s_s);
}

__global__ __launch_bounds__(256) void mip_apply_bwd_kernel(int64_t G, const float* __restrict__ scales, const float* __restrict__ opac,
                                                            const float* __restrict__ filter, const float* __restrict__ g_scales_f,
                                                            const float* __restrict__ g_opac_f, float* __restrict__ g_scales, float* __restrict__ g_opac) {
  __shared__ float s_s[768], s_g[768];
  rows3_load(scales, G, s_s);
  rows3_load(g_scales_f, G, s_g);
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = gi < G;
  const float s[3] = {s_s[3 * threadIdx.x], s_s[3 * threadIdx.x + 1], s_s[3 * threadIdx.x + 2]};
  const float gs[3] = {s_g[3 * threadIdx.x], s_g[3 * threadIdx.x + 1], s_g[3 * threadIdx.x + 2]};
  const float f = live ? filter[gi] : 0.f, o = live ? opac[gi] : 0.f, go = live ? g_opac_f[gi] : 0.f;
  float sf[3], q[3];
  mip_axes(s, f, sf, q);
  if (live) g_opac[gi] = go * ((q[0] * q[1]) * q[2]);
  const float rest[3] = {q[1] * q[2], q[0] * q[2], q[0] * q[1]};
  const float w = go * o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float r = 0.f;
    if (sf[i] > 0.f) {
      const float fs = f / sf[i];
      const float dq = (fs * fs) / sf[i];  // d q_i / d |s_i| = f^2 / sf_i^3
      r = gs[i] * (s[i] / sf[i]) + (w * rest[i]) * (s[i] < 0.f ? -dq : dq);
    }
    s_g[3 * threadIdx.x + i] = r;
  }
  rows3_store(g_scales, G, s_g);
}

}  // namespace

extern "C" int64_t siu3r_mip_filter3d_ws(int V) { return V > 0 ? (int64_t)sizeof(float) * (MIP_WS_CAM * (int64_t)V + 4) : 0; }

extern "C" int siu3r_mip_filter3d(const float* c2w_dev, const float* Kn_dev, int V, int width, int height, const float* means, int64_t G, float z_near,
                                  float margin, float variance, float* filter, void* ws, void* stream) {
  SIU3R_CHECK(V >= 1 && V <= 65535 && width > 0 && height > 0, "mip_filter3d: bad view count or frame size (V = %d, %d x %d)", V, width, height);
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "mip_filter3d: G = %ld out of range", (long)G);
  SIU3R_CHECK(c2w_dev && Kn_dev && ws && (G == 0 || (means && filter)), "mip_filter3d: null pointer");
  SIU3R_CHECK(((uintptr_t)ws & 3) == 0, "mip_filter3d: the workspace must be 4-byte aligned");
  SIU3R_CHECK(z_near >= 0.f && margin >= 0.f && variance > 0.f && variance < 3.0e38f && z_near < 3.0e38f && margin < 3.0e38f,
              "mip_filter3d: z_near >= 0, margin >= 0 and variance > 0 (finite) are required");
  if (G == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  float* wsf = (float*)ws;
  unsigned int* dmax = (unsigned int*)(wsf + MIP_WS_CAM * (int64_t)V);
  if (hipMemsetAsync(dmax, 0, sizeof(unsigned int), s) != hipSuccess) {
    siu3r_set_error("mip_filter3d: memset failed");
    return 2;
  }
  hipLaunchKernelGGL(mip_cams_kernel, dim3((V + 63) / 64), dim3(64), 0, s, V, width, height, c2w_dev, Kn_dev, wsf);
  const dim3 grid((unsigned)cdiv64(G, 256));
  hipLaunchKernelGGL(mip_depth_kernel, grid, dim3(256), 0, s, V, width, height, G, means, z_near, margin, (const float*)wsf, filter, dmax);
  hipLaunchKernelGGL(mip_finish_kernel, grid, dim3(256), 0, s, V, G, variance, (const float*)wsf, (const unsigned int*)dmax, filter);
  SIU3R_LAUNCH_CHECK("siu3r_mip_filter3d");
  return 0;
}

extern "C" int siu3r_mip_apply(const float* scales, const float* opacities, const float* filter, int64_t G, float* scales_f, float* opac_f, void* stream) {
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "mip_apply: G = %ld out of range", (long)G);
  SIU3R_CHECK(G == 0 || (scales && opacities && filter && scales_f && opac_f), "mip_apply: null pointer");
  if (G == 0) return 0;
  hipLaunchKernelGGL(mip_apply_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, (hipStream_t)stream, G, scales, opacities, filter, scales_f, opac_f);
  SIU3R_LAUNCH_CHECK("siu3r_mip_apply");
  return 0;
}

extern "C" int siu3r_mip_apply_bwd(const float* scales, const float* opacities, const float* filter, const float* g_scales_f, const float* g_opac_f, int64_t G,
                                   float* g_scales, float* g_opac, void* stream) {
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "mip_apply_bwd: G = %ld out of range", (long)G);
  SIU3R_CHECK(G == 0 || (scales && opacities && filter && g_scales_f && g_opac_f && g_scales && g_opac), "mip_apply_bwd: null pointer");
  if (G == 0) return 0;
  hipLaunchKernelGGL(mip_apply_bwd_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, (hipStream_t)stream, G, scales, opacities, filter, g_scales_f, g_opac_f,
                     g_scales, g_opac);
  SIU3R_LAUNCH_CHECK("siu3r_mip_apply_bwd");
  return 0;
}
