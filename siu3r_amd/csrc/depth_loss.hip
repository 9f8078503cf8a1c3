// Fused depth loss of splat refinement: value AND gradient w.r.t. the K2 render's depth (D = sum w z) and opacity
// (O = sum w) maps against a target depth T with an optional per-pixel confidence Wt, all fp32 [V,H,W], contiguous.
//
// A pixel is valid iff O > min_opacity, D > 0, T > 0, Wt > 0 (when given) and all of them are finite; every comparison is false for a NaN.
// An invalid pixel adds nothing to any sum and gets +0 in both gradient maps.  At a valid pixel, in fp64 (an upcast of fp32 is exact):
//   space 0 (depth):    x = D / O, y = T,     dx/dD = 1 / O,     dx/dO = -D / O^2
//   space 1 (inverse):  x = O / D, y = 1 / T, dx/dD = -O / D^2,  dx/dO = 1 / D
//   mode 0 (l1):      loss = sum w |x - y| / N, N = sum w over all views; ONE pass writes the partial sums and the gradient WITHOUT the
//                     factor 1 / N, which the finalize kernel leaves in out[2] for the caller's multiply
//   mode 1 (pearson): per view rho = sxy / sqrt(sxx syy) of the w-weighted moments; loss = mean of 1 - rho over the counted views (at least
//                     two valid pixels, max x > min x, max y > min y).  Moments pass -> finalize -> gradient pass.
// 1 - rho of smooth depth is ~4e-4 built from second moments of values around 3: x, y and the six raw moments are fp64 from the pixel on
// (the kernels stay bound by memory: four planes in, two out).
// Work split: a workgroup (256 threads, 4 pixels each, 16-byte accesses where the plane's base allows) owns 1,024 pixels of ONE view; it
// reduces by a fixed shuffle tree per wave, then the four waves in index order, and writes one record of REC doubles.  One workgroup then
// adds the records of each view in a fixed order (chunks of 256).  No atomics: two calls give the same bits.
#include "block_reduce.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int PX = 4;            // pixels per thread
constexpr int CHUNK = NT * PX;   // pixels per workgroup
constexpr int REC = 11;          // doubles per record: count, sw, then l1: s|x-y| / pearson: swx, swy, swxx, swyy, swxy, min x, max x, min y, max y
constexpr int NSTAT = 4;         // doubles per view for the gradient pass: mu_x, mu_y, c_y, c_x
constexpr float FMAX = 3.402823466e+38f;

struct DepthArgs {
  const float* depth;
  const float* opacity;
  const float* target;
  const float* weight;  // or null
  float* g_depth;       // both or neither
  float* g_opacity;
  double* partials;     // [V, bpv, REC]
  double* stats;        // [V, NSTAT]
  int P, bpv, inverse;
  float min_opacity;
};

// PX consecutive values of one plane; `fill` past the end of the plane
__device__ inline void load_px(const float* plane, int i0, int P, bool vec, float fill, float (&v)[PX]) {
  if (vec && i0 + PX <= P) {
    const float4 q = *reinterpret_cast<const float4*>(plane + i0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) v[k] = i0 + k < P ? plane[i0 + k] : fill;
  }
}

__device__ inline void store_px(float* plane, int i0, int P, bool vec, const float (&v)[PX]) {
  if (vec && i0 + PX <= P) {
    *reinterpret_cast<float4*>(plane + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k)
      if (i0 + k < P) plane[i0 + k] = v[k];
  }
}

// the workgroup's pixels of its view in fp64
struct Pixels {
  bool ok[PX];
  double x[PX], y[PX], w[PX], dxdD[PX], dxdO[PX];
  int i0;
  bool vec;
  int64_t base;
};

__device__ inline void load_pixels(const DepthArgs& a, Pixels& p) {
  p.base = (int64_t)blockIdx.y * a.P;
  p.i0 = blockIdx.x * CHUNK + threadIdx.x * PX;
  // one decision per workgroup: the chunk starts a multiple of 4 KiB into the plane, so only the plane's base matters
  p.vec = aligned16(a.depth + p.base) && aligned16(a.opacity + p.base) && aligned16(a.target + p.base) && (!a.weight || aligned16(a.weight + p.base)) &&
          (!a.g_depth || (aligned16(a.g_depth + p.base) && aligned16(a.g_opacity + p.base)));
  float d[PX], o[PX], t[PX], w[PX];
  load_px(a.depth + p.base, p.i0, a.P, p.vec, 0.f, d);
  load_px(a.opacity + p.base, p.i0, a.P, p.vec, 0.f, o);  // (past the end: O = 0 <= min_opacity, invalid)
  load_px(a.target + p.base, p.i0, a.P, p.vec, 0.f, t);
  if (a.weight) {
    load_px(a.weight + p.base, p.i0, a.P, p.vec, 0.f, w);
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) w[k] = 1.f;
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    p.ok[k] = o[k] > a.min_opacity && o[k] <= FMAX && d[k] > 0.f && d[k] <= FMAX && t[k] > 0.f && t[k] <= FMAX && w[k] > 0.f && w[k] <= FMAX;
    const double D = p.ok[k] ? (double)d[k] : 1.0, O = p.ok[k] ? (double)o[k] : 1.0, T = p.ok[k] ? (double)t[k] : 1.0;
    if (a.inverse) {
      const double iD = 1.0 / D;
      p.x[k] = O * iD;
      p.y[k] = 1.0 / T;
      p.dxdD[k] = -p.x[k] * iD;
      p.dxdO[k] = iD;
    } else {
      const double iO = 1.0 / O;
      p.x[k] = D * iO;
      p.y[k] = T;
      p.dxdD[k] = iO;
      p.dxdO[k] = -p.x[k] * iO;
    }
    p.w[k] = (double)w[k];
  }
}

// mode l1: sums and, with GRAD, the gradient without its 1 / N
template <bool GRAD>
__global__ __launch_bounds__(NT) void depth_l1_kernel(DepthArgs a) {
  __shared__ double red[3 * 4];
  Pixels p;
  load_pixels(a, p);
  double s[3] = {0.0, 0.0, 0.0};
  float gd[PX], go[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    gd[k] = go[k] = 0.f;
    if (p.ok[k]) {
      const double e = p.x[k] - p.y[k];
      s[0] += 1.0;
      s[1] += p.w[k];
      s[2] += p.w[k] * fabs(e);
      if (GRAD) {
        const double g = e > 0.0 ? p.w[k] : (e < 0.0 ? -p.w[k] : 0.0);
        gd[k] = (float)(g * p.dxdD[k]);
        go[k] = (float)(g * p.dxdO[k]);
      }
    }
  }
  if (GRAD) {
    store_px(a.g_depth + p.base, p.i0, a.P, p.vec, gd);
    store_px(a.g_opacity + p.base, p.i0, a.P, p.vec, go);
  }
  block_reduce<Reduce::Sum>(s, red);
  if (threadIdx.x == 0) {
    double* r = a.partials + ((int64_t)blockIdx.y * a.bpv + blockIdx.x) * REC;
    r[0] = s[0], r[1] = s[1], r[2] = s[2];
  }
}

// mode pearson, first pass: the record of the workgroup's valid pixels
__global__ __launch_bounds__(NT) void depth_moments_kernel(DepthArgs a) {
  __shared__ double red[7 * 4];
  Pixels p;
  load_pixels(a, p);
  const double inf = __builtin_inf();
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lo[2] = {inf, inf}, hi[2] = {-inf, -inf};
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    if (p.ok[k]) {
      const double w = p.w[k], x = p.x[k], y = p.y[k];
      s[0] += 1.0;
      s[1] += w;
      s[2] += w * x;
      s[3] += w * y;
      s[4] += w * x * x;
      s[5] += w * y * y;
      s[6] += w * x * y;
      lo[0] = fmin(lo[0], x), hi[0] = fmax(hi[0], x);
      lo[1] = fmin(lo[1], y), hi[1] = fmax(hi[1], y);
    }
  }
  block_reduce<Reduce::Sum>(s, red);
  block_reduce<Reduce::Min>(lo, red);
  block_reduce<Reduce::Max>(hi, red);
  if (threadIdx.x == 0) {
    double* r = a.partials + ((int64_t)blockIdx.y * a.bpv + blockIdx.x) * REC;
#pragma unroll
    for (int k = 0; k < 7; ++k) r[k] = s[k];
    r[7] = lo[0], r[8] = hi[0], r[9] = lo[1], r[10] = hi[1];
  }
}

// mode pearson, last pass: d loss / dx = w [ (y - mu_y) c_y + (x - mu_x) c_x ] with the view's four numbers from the finalize kernel
// (c_y = c_x = 0 for a view that is not counted)
__global__ __launch_bounds__(NT) void depth_pearson_grad_kernel(DepthArgs a) {
  Pixels p;
  load_pixels(a, p);
  const double* st = a.stats + (int64_t)blockIdx.y * NSTAT;
  const double mx = st[0], my = st[1], cy = st[2], cx = st[3];
  const bool counted = cy != 0.0 || cx != 0.0;
  float gd[PX], go[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    gd[k] = go[k] = 0.f;
    if (p.ok[k] && counted) {
      const double g = p.w[k] * ((p.y[k] - my) * cy + (p.x[k] - mx) * cx);
      gd[k] = (float)(g * p.dxdD[k]);
      go[k] = (float)(g * p.dxdO[k]);
    }
  }
  store_px(a.g_depth + p.base, p.i0, a.P, p.vec, gd);
  store_px(a.g_opacity + p.base, p.i0, a.P, p.vec, go);
}

// one workgroup: per view, thread t adds the records t, t + 256, ... in that order, then the fixed tree; the views in index order.
// out = (loss, N or the number of counted views, the factor the caller's gradient multiply still owes, 0)
__global__ __launch_bounds__(NT) void depth_finalize_kernel(const double* partials, int V, int bpv, int pearson, double* stats, float* out,
                                                            float* per_view, int32_t* valid) {
  __shared__ double red[7 * 4];
  const float nan = __builtin_nanf("");
  const double inf = __builtin_inf();
  double total = 0.0, denom = 0.0;  // l1: sum w |x - y|, sum w;  pearson: sum (1 - rho), counted views
  for (int v = 0; v < V; ++v) {
    const double* pv = partials + (int64_t)v * bpv * REC;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lo[2] = {inf, inf}, hi[2] = {-inf, -inf};
    for (int i = threadIdx.x; i < bpv; i += NT) {
      const double* r = pv + (int64_t)i * REC;
      s[0] += r[0], s[1] += r[1], s[2] += r[2];
      if (pearson) {
        s[3] += r[3], s[4] += r[4], s[5] += r[5], s[6] += r[6];
        lo[0] = fmin(lo[0], r[7]), hi[0] = fmax(hi[0], r[8]);
        lo[1] = fmin(lo[1], r[9]), hi[1] = fmax(hi[1], r[10]);
      }
    }
    block_reduce<Reduce::Sum>(s, red);
    if (pearson) {
      block_reduce<Reduce::Min>(lo, red);
      block_reduce<Reduce::Max>(hi, red);
    }
    // every thread holds the same totals; thread 0 writes
    if (!pearson) {
      total += s[2];
      denom += s[1];
      if (threadIdx.x == 0) {
        valid[v] = (int32_t)s[0];
        per_view[v] = s[0] > 0.0 ? (float)(s[2] / s[1]) : nan;
      }
    } else {
      const bool counted = s[0] >= 2.0 && hi[0] > lo[0] && hi[1] > lo[1];
      double mx = 0.0, my = 0.0, cy = 0.0, cx = 0.0, one_minus_rho = 0.0;
      if (counted) {
        const double isw = 1.0 / s[1];
        mx = s[2] * isw, my = s[3] * isw;
        const double sxx = s[4] * isw - mx * mx, syy = s[5] * isw - my * my, sxy = s[6] * isw - mx * my;
        const double inorm = 1.0 / sqrt(sxx * syy);
        const double rho = sxy * inorm;
        one_minus_rho = 1.0 - rho;
        cy = -inorm * isw;
        cx = rho / sxx * isw;
        total += one_minus_rho;
        denom += 1.0;
      }
      if (threadIdx.x == 0) {
        valid[v] = (int32_t)s[0];
        per_view[v] = counted ? (float)one_minus_rho : nan;
        double* st = stats + (int64_t)v * NSTAT;
        st[0] = mx, st[1] = my, st[2] = cy, st[3] = cx;
      }
    }
  }
  if (threadIdx.x == 0) {
    const double inv = denom > 0.0 ? 1.0 / denom : 0.0;
    out[0] = (float)(total * inv);
    out[1] = (float)denom;
    out[2] = pearson ? 1.f : (float)inv;
    out[3] = 0.f;
    if (pearson)  // the mean over the counted views, folded into the gradient pass's two factors
      for (int v = 0; v < V; ++v) stats[(int64_t)v * NSTAT + 2] *= inv, stats[(int64_t)v * NSTAT + 3] *= inv;
  }
}

int blocks_per_view(int H, int W) { return (int)(((int64_t)H * W + CHUNK - 1) / CHUNK); }

}  // namespace

extern "C" int64_t siu3r_depth_loss_ws(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff - CHUNK) return 0;
  return ((int64_t)V * blocks_per_view(H, W) * REC + (int64_t)V * NSTAT) * (int64_t)sizeof(double);
}

extern "C" int siu3r_depth_loss(const float* depth, const float* opacity, const float* target, const float* weight, int V, int H, int W, int mode,
                                int space, float min_opacity, float* g_depth, float* g_opacity, void* ws, float* out, float* per_view, int32_t* valid,
                                void* stream) {
  SIU3R_CHECK(depth && opacity && target && ws && out && per_view && valid, "depth_loss: null pointer");
  SIU3R_CHECK(V > 0 && H > 0 && W > 0, "depth_loss: empty input [%d,%d,%d]", V, H, W);
  SIU3R_CHECK((int64_t)H * W <= 0x7fffffff - CHUNK, "depth_loss: %d x %d pixels per view exceed 32-bit indexing", H, W);
  SIU3R_CHECK(V <= 65535, "depth_loss: %d views exceed one launch", V);
  SIU3R_CHECK(mode == 0 || mode == 1, "depth_loss: mode %d (0 l1, 1 pearson)", mode);
  SIU3R_CHECK(space == 0 || space == 1, "depth_loss: space %d (0 depth, 1 inverse)", space);
  SIU3R_CHECK(min_opacity >= 0.f && min_opacity <= FMAX, "depth_loss: min_opacity %g must be finite and >= 0", (double)min_opacity);
  SIU3R_CHECK((g_depth == nullptr) == (g_opacity == nullptr), "depth_loss: g_depth and g_opacity come together");
  SIU3R_CHECK(((uintptr_t)ws & 7) == 0, "depth_loss: the workspace must be 8-byte aligned");
  DepthArgs a;
  a.depth = depth, a.opacity = opacity, a.target = target, a.weight = weight;
  a.g_depth = g_depth, a.g_opacity = g_opacity;
  a.P = H * W;
  a.bpv = blocks_per_view(H, W);
  a.partials = (double*)ws;
  a.stats = a.partials + (int64_t)V * a.bpv * REC;
  a.inverse = space;
  a.min_opacity = min_opacity;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)a.bpv, (unsigned)V);
  if (mode == 1)
    hipLaunchKernelGGL(depth_moments_kernel, grid, dim3(NT), 0, s, a);
  else if (g_depth)
    hipLaunchKernelGGL(depth_l1_kernel<true>, grid, dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(depth_l1_kernel<false>, grid, dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_depth_loss");
  hipLaunchKernelGGL(depth_finalize_kernel, dim3(1), dim3(NT), 0, s, (const double*)a.partials, V, a.bpv, mode, a.stats, out, per_view, valid);
  SIU3R_LAUNCH_CHECK("siu3r_depth_loss (final sum)");
  if (mode == 1 && g_depth) {
    hipLaunchKernelGGL(depth_pearson_grad_kernel, grid, dim3(NT), 0, s, a);
    SIU3R_LAUNCH_CHECK("siu3r_depth_loss (gradient)");
  }
  return 0;
}
