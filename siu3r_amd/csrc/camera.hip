// The cameras of splat refinement: a per-view colour transform with its gradients, and ONE launch that steps every
// camera's pose and colour transform.
//
// Exposure.  out[v,c,p] = sum_k M[v,c,k] in[v,k,p] + M[v,c,3], M [V,3,4] fp32.  `in` is read as stored through four element strides (view,
// channel, row, column), `out` and `g_out` are contiguous [V,3,H,W].  Backward: g_in[v,k,p] = sum_c M[v,c,k] g_out[v,c,p] in in's layout,
// g_M[v,c,k] = sum_p g_out[v,c,p] in[v,k,p], g_M[v,c,3] = sum_p g_out[v,c,p].  A pixel's three channels are read once and feed all nine
// products.  Both kernels are streams: a workgroup (256 threads, 2 rounds of 4 consecutive pixels each) owns 2,048 pixels of ONE view; 16-byte
// accesses where the layout is dense planes ([V,3,H,W]) or dense pixels ([V,H,W,3]) on 16-byte aligned bases, scalar accesses through the
// strides otherwise.  The twelve sums per view: fp64 products (exact) added per thread, the fixed tree of block_reduce.h per workgroup, one
// record of 12 doubles per workgroup, and a small second launch that adds the records of a view in index order.  No atomics: two calls give
// the same bits.  The transform is a pass of its own and not part of photo_ssim_kernel: that kernel owns one (view, channel) plane per
// workgroup, so mixing channels there would read every plane three times and g_in would need sums across workgroups.
//
// Camera step.  One thread per view, everything in fp64 from the fp32 state and rounded once on store (V x 18 values).  Adam in the
// operation order of gaussian_adam.hip on xi = (rho, theta), which is re-centred at 0 every step, and on M:
//   m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  step = ((lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps);  xi = -step;  M -= step
// and the retraction c2w <- c2w exp(-xi^) (a left perturbation of world->camera, pose_align.align_pose) in closed form,
//   exp(u^) = [R t; 0 1],  R = I + A K + B K^2,  t = (I + B K + C K^2) rho,  K = theta^,
//   A = sin th / th,  B = (1 - cos th) / th^2,  C = (th - sin th) / th^3,  three-term series of all three below th = 1e-2
// (that switch point agrees with the matrix exponential to 4e-15 over 0 .. 3; 1e-3 loses two digits to the cancellation in B and C).
// A view whose `free` byte is 0 is not written.  A free view whose update is exactly zero keeps the bits of c2w: the product with the
// identity is not formed (it would turn a -0 entry into +0).
#include "image_io.h"

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int ROUNDS = 2;
constexpr int CHUNK = NT * PX * ROUNDS;  // pixels per workgroup
constexpr int REC = 12;                  // doubles per record: g_M of the workgroup's pixels, row-major [3][4]

struct ExpArgs {
  const float* in;
  const float* M;
  const float* g_out;
  float* out;
  float* g_in;
  double* partials;  // [V, bpv, REC]
  int64_t s[4];      // element strides of `in` (and g_in): view, channel, row, column
  int W, P, bpv, layout;
};

__global__ __launch_bounds__(NT) void exposure_fwd_kernel(ExpArgs a) {
  const int v = blockIdx.y;
  float M[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = a.M[v * 12 + k];
  const float* in = a.in + v * a.s[0];
  float* out = a.out + (int64_t)v * 3 * a.P;
  const bool vin = strided_vec(in, a), vout = planes_vec(out, a.P);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i0 = blockIdx.x * CHUNK + r * NT * PX + threadIdx.x * PX;
    if (i0 >= a.P) break;
    float x[3][PX], y[3][PX];
    load3(in, a, i0, vin, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < PX; ++k) y[c][k] = fmaf(M[4 * c + 2], x[2][k], fmaf(M[4 * c + 1], x[1][k], fmaf(M[4 * c], x[0][k], M[4 * c + 3])));
    }
    store_planes(out, a.P, i0, vout, y);
  }
}

// GIN: g_in is written; GM: the workgroup's record of g_M is written (and only then `in` is read)
template <bool GIN, bool GM>
__global__ __launch_bounds__(NT) void exposure_bwd_kernel(ExpArgs a) {
  __shared__ double red[GM ? REC * 4 : 1];
  const int v = blockIdx.y;
  float M[12];
  if (GIN) {
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = a.M[v * 12 + k];
  }
  const float* in = a.in + v * a.s[0];
  float* g_in = GIN ? a.g_in + v * a.s[0] : nullptr;
  const float* g_out = a.g_out + (int64_t)v * 3 * a.P;
  const bool vin = GM && strided_vec(in, a), vgin = GIN && strided_vec(g_in, a), vg = planes_vec(g_out, a.P);
  double s[REC];
#pragma unroll
  for (int k = 0; k < REC; ++k) s[k] = 0.0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i0 = blockIdx.x * CHUNK + r * NT * PX + threadIdx.x * PX;
    if (i0 >= a.P) break;
    float g[3][PX];
    load_planes(g_out, a.P, i0, vg, g);
    if (GM) {
      float x[3][PX];
      load3(in, a, i0, vin, x);  // (0 past the end, as g: those pixels add nothing)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          const double gc = (double)g[c][k];
          s[4 * c] = fma(gc, (double)x[0][k], s[4 * c]);  // (the product of two floats is exact in fp64: the same bits as multiply, then add)
          s[4 * c + 1] = fma(gc, (double)x[1][k], s[4 * c + 1]);
          s[4 * c + 2] = fma(gc, (double)x[2][k], s[4 * c + 2]);
          s[4 * c + 3] += gc;
        }
      }
    }
    if (GIN) {
      float gi[3][PX];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < PX; ++k) gi[j][k] = fmaf(M[8 + j], g[2][k], fmaf(M[4 + j], g[1][k], M[j] * g[0][k]));
      }
      store3(g_in, a, i0, vgin, gi);
    }
  }
  if (GM) {
    block_reduce<Reduce::Sum>(s, red);
    if (threadIdx.x == 0) {
      double* rec = a.partials + ((int64_t)v * a.bpv + blockIdx.x) * REC;
#pragma unroll
      for (int k = 0; k < REC; ++k) rec[k] = s[k];
    }
  }
}

// one thread per entry of g_M: the records of its view in index order.  The loads of GB records are issued together and then added one
// after the other (a load per add would make the launch a chain of bpv memory latencies: 31 us at 6 x 512 x 512, twice the pass itself)
__global__ __launch_bounds__(NT) void exposure_gm_kernel(const double* partials, int V, int bpv, float* g_M) {
  constexpr int GB = 32;
  for (int e = blockIdx.x * NT + threadIdx.x; e < V * REC; e += gridDim.x * NT) {
    const int v = e / REC, k = e - v * REC;
    const double* rec = partials + (int64_t)v * bpv * REC + k;
    double s = 0.0;
    for (int i0 = 0; i0 < bpv; i0 += GB) {
      double r[GB];
#pragma unroll
      for (int j = 0; j < GB; ++j) r[j] = i0 + j < bpv ? rec[(int64_t)(i0 + j) * REC] : 0.0;  // (s + 0 is s)
#pragma unroll
      for (int j = 0; j < GB; ++j) s += r[j];
    }
    g_M[e] = (float)s;
  }
}

int blocks_per_view(int H, int W) { return (int)(((int64_t)H * W + CHUNK - 1) / CHUNK); }

// what both exposure entry points check and derive
int exposure_args(const char* who, const float* in, const int64_t* st, const float* M, int V, int H, int W, ExpArgs& a) {
  SIU3R_CHECK(in && st && M, "%s: null pointer", who);
  SIU3R_CHECK(V > 0 && H > 0 && W > 0, "%s: empty input [%d,3,%d,%d]", who, V, H, W);
  SIU3R_CHECK((int64_t)H * W <= 0x7fffffff - CHUNK, "%s: %d x %d pixels per view exceed 32-bit indexing", who, H, W);
  SIU3R_CHECK(V <= 65535, "%s: %d views exceed one launch", who, V);
  for (int i = 0; i < 4; ++i) SIU3R_CHECK(st[i] >= 0, "%s: negative strides are not supported", who);
  memset(&a, 0, sizeof(a));
  a.in = in, a.M = M;
  for (int i = 0; i < 4; ++i) a.s[i] = st[i];
  a.W = W, a.P = H * W;
  a.bpv = blocks_per_view(H, W);
  const bool rows_dense = H == 1 || st[2] == (int64_t)W * st[3];
  a.layout = st[3] == 1 && rows_dense ? PLANES : (st[1] == 1 && st[3] == 3 && rows_dense ? PIXELS : STRIDED);
  return 0;
}

// ---- the camera step ----------------------------------------------------------------------------------------------------------------

struct CamArgs {
  float* c2w;            // [V,4,4] or null
  const float* g_xi;     // [V,6] (rho, theta)
  float* M;              // [V,3,4] or null
  const float* g_M;      // [V,3,4]
  float* m1;             // [V,18]: 6 of the pose, 12 of the exposure
  float* m2;
  const uint8_t* free_;  // [V] or null (every view is free)
  int V;
  double lr_trans, lr_rot, lr_exposure;  // each already divided by bc1
  double b1, omb1, b2, omb2, eps, bc2s;
};

// one Adam update in fp64 from the fp32 moments, which are rounded once on store; returns the step to subtract
__device__ inline double adam_step64(const CamArgs& a, double g, float* m1, float* m2, double lr_bc1) {
  const double m = a.b1 * (double)*m1 + a.omb1 * g;
  const double v = a.b2 * (double)*m2 + (a.omb2 * g) * g;
  *m1 = (float)m;
  *m2 = (float)v;
  return (lr_bc1 * m) / (sqrt(v) / a.bc2s + a.eps);
}

__global__ __launch_bounds__(64) void camera_step_kernel(CamArgs a) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= a.V || (a.free_ && a.free_[v] == 0)) return;
  float* m1 = a.m1 + v * 18;
  float* m2 = a.m2 + v * 18;
  if (a.c2w) {
    double u[6];  // -xi: c2w <- c2w exp(u^)
    bool moves = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      u[k] = adam_step64(a, (double)a.g_xi[v * 6 + k], m1 + k, m2 + k, k < 3 ? a.lr_trans : a.lr_rot);
      moves = moves || !(u[k] == 0.0);
    }
    if (moves) {
      const double wx = u[3], wy = u[4], wz = u[5];
      const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
      double A, B, C;
      if (th < 1e-2) {
        A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
        C = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
      } else {
        const double sn = sin(th), cs = cos(th);
        A = sn / th;
        B = (1.0 - cs) / th2;
        C = (th - sn) / (th2 * th);
      }
      const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
      const double w[3] = {wx, wy, wz};
      double E[4][4];  // exp(u^)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double K2 = w[i] * w[j] - (i == j ? th2 : 0.0), I = i == j ? 1.0 : 0.0;
          E[i][j] = I + A * K[i][j] + B * K2;
          t += (I + B * K[i][j] + C * K2) * u[j];
        }
        E[i][3] = t;
      }
      E[3][0] = E[3][1] = E[3][2] = 0.0, E[3][3] = 1.0;
      float* c = a.c2w + v * 16;
      double P[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) P[i][j] = (double)c[4 * i + j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[4 * i + j] = (float)(P[i][0] * E[0][j] + P[i][1] * E[1][j] + P[i][2] * E[2][j] + P[i][3] * E[3][j]);
      }
    }
  }
  if (a.M) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const double step = adam_step64(a, (double)a.g_M[v * 12 + k], m1 + 6 + k, m2 + 6 + k, a.lr_exposure);
      a.M[v * 12 + k] = (float)((double)a.M[v * 12 + k] - step);
    }
  }
}

}  // namespace

extern "C" int64_t siu3r_exposure_ws(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff - CHUNK) return 0;
  return (int64_t)V * blocks_per_view(H, W) * REC * (int64_t)sizeof(double);
}

extern "C" int siu3r_exposure_apply(const float* in, const int64_t* in_strides, const float* M, int V, int H, int W, float* out, void* stream) {
  ExpArgs a;
  if (int rc = exposure_args("exposure_apply", in, in_strides, M, V, H, W, a)) return rc;
  SIU3R_CHECK(out, "exposure_apply: null pointer");
  a.out = out;
  hipLaunchKernelGGL(exposure_fwd_kernel, dim3((unsigned)a.bpv, (unsigned)V), dim3(NT), 0, (hipStream_t)stream, a);
  SIU3R_LAUNCH_CHECK("siu3r_exposure_apply");
  return 0;
}

extern "C" int siu3r_exposure_apply_bwd(const float* in, const int64_t* in_strides, const float* M, const float* g_out, int V, int H, int W, float* g_in,
                                        float* g_M, void* ws, void* stream) {
  ExpArgs a;
  if (int rc = exposure_args("exposure_apply_bwd", in, in_strides, M, V, H, W, a)) return rc;
  SIU3R_CHECK(g_out, "exposure_apply_bwd: null pointer");
  SIU3R_CHECK(!g_M || (ws && ((uintptr_t)ws & 7) == 0), "exposure_apply_bwd: g_M needs the workspace (siu3r_exposure_ws bytes, 8-byte aligned)");
  if (!g_in && !g_M) return 0;
  a.g_out = g_out, a.g_in = g_in, a.partials = (double*)ws;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)a.bpv, (unsigned)V);
  if (g_in && g_M)
    hipLaunchKernelGGL((exposure_bwd_kernel<true, true>), grid, dim3(NT), 0, s, a);
  else if (g_in)
    hipLaunchKernelGGL((exposure_bwd_kernel<true, false>), grid, dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL((exposure_bwd_kernel<false, true>), grid, dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_exposure_apply_bwd");
  if (g_M) {
    hipLaunchKernelGGL(exposure_gm_kernel, dim3((unsigned)((V * REC + NT - 1) / NT)), dim3(NT), 0, s, (const double*)a.partials, V, a.bpv, g_M);
    SIU3R_LAUNCH_CHECK("siu3r_exposure_apply_bwd (final sum)");
  }
  return 0;
}

extern "C" int siu3r_camera_step(float* c2w, const float* g_xi, float* M, const float* g_M, float* exp_avg, float* exp_avg_sq, const uint8_t* free_mask,
                                 int V, int64_t t, double lr_trans, double lr_rot, double lr_exposure, double beta1, double beta2, double eps, void* stream) {
  SIU3R_CHECK(V > 0 && V <= (1 << 24), "camera_step: %d views", V);
  SIU3R_CHECK(t >= 1, "camera_step: step count %lld must be >= 1", (long long)t);
  SIU3R_CHECK((c2w == nullptr) == (g_xi == nullptr), "camera_step: c2w and g_xi come together");
  SIU3R_CHECK((M == nullptr) == (g_M == nullptr), "camera_step: M and g_M come together");
  SIU3R_CHECK(c2w || M, "camera_step: neither the pose nor the exposure half is given");
  SIU3R_CHECK(exp_avg && exp_avg_sq, "camera_step: null moments");
  SIU3R_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "camera_step: betas (%g, %g) must lie in [0, 1)", beta1, beta2);
  SIU3R_CHECK(eps >= 0.0 && eps < 1e300, "camera_step: eps %g must be finite and >= 0", eps);
  SIU3R_CHECK(lr_trans >= 0.0 && lr_rot >= 0.0 && lr_exposure >= 0.0 && lr_trans + lr_rot + lr_exposure < 1e300,
              "camera_step: a negative or non-finite rate (%g, %g, %g)", lr_trans, lr_rot, lr_exposure);
  CamArgs a;
  a.c2w = c2w, a.g_xi = g_xi, a.M = M, a.g_M = g_M, a.m1 = exp_avg, a.m2 = exp_avg_sq, a.free_ = free_mask, a.V = V;
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  a.lr_trans = lr_trans / bc1, a.lr_rot = lr_rot / bc1, a.lr_exposure = lr_exposure / bc1;
  a.b1 = beta1, a.omb1 = 1.0 - beta1, a.b2 = beta2, a.omb2 = 1.0 - beta2, a.eps = eps, a.bc2s = sqrt(bc2);
  hipLaunchKernelGGL(camera_step_kernel, dim3((unsigned)((V + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  SIU3R_LAUNCH_CHECK("siu3r_camera_step");
  return 0;
}
