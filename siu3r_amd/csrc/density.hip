// Adaptive density control of splat refinement (Kerbl et al. 2023, section 5.2): per-Gaussian statistics every
// iteration, and at an event a plan (one action and one output count per Gaussian, an order-preserving exclusive scan of the counts) and
// an apply (a gather of every parameter row and its two Adam moments into freshly sized arrays).
//
//   accumulate  one thread per Gaussian walks the views in index order: the NDC-scaled norm of the pixel-space mean gradient, the number
//               of views that saw the Gaussian, the largest screen radius.  Visibility is radii > 0, never the gradient's value (the
//               projection backward does not write the rows of culled Gaussians).
//   plan        plan_action_kernel (action + per-workgroup sums of output rows / pruned / cloned / split)
//               -> plan_sums_kernel (ONE workgroup: exclusive scan of the workgroup sums, totals)
//               -> plan_offset_kernel (scan inside the workgroup + its base).  Integer throughout: the offsets are exact and the same on
//               every call.  Output rows of Gaussian g are offset[g] .. offset[g] + count - 1: the set keeps its memory order.
//   apply       one launch per field; lanes run along the row ELEMENTS (thread t owns element t % r of source row t / r), so that a
//               75-float harmonics row is read and written by consecutive lanes.  keep: the bits; clone: the bits twice, the copy with zero
//               moments; split: two children (means: + R(q / |q|) (exp(log_scale) o z), log-scales: - log 1.6), zero moments.
// No kernel holds a float atomic, none allocates or synchronises with the host.
#include "gaussian_shared.h"

namespace {

constexpr int NT = 256;       // threads per workgroup of every kernel but the scan of the workgroup sums
constexpr int NT_SUMS = 1024;
enum { PRUNE = 0, KEEP = 1, CLONE = 2, SPLIT = 3 };  // output rows = min(action, 2)
constexpr float LOG_SPLIT = 0.47000362924573563f;    // log(1.6): children have scale / (0.8 * 2)

__global__ __launch_bounds__(NT) void accumulate_kernel(const float* __restrict__ g_mean2d, const int32_t* __restrict__ radii, int V, int64_t G, float sx,
                                                        float sy, float* __restrict__ grad_accum, int32_t* __restrict__ seen,
                                                        int32_t* __restrict__ max_radius) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= G) return;
  float acc = grad_accum[g];
  int n = seen[g], rmax = max_radius[g];
  for (int v = 0; v < V; ++v) {
    const int64_t o = (int64_t)v * G + g;
    const int2 r = *(const int2*)(radii + 2 * o);
    if (r.x > 0 || r.y > 0) {
      const float2 d = *(const float2*)(g_mean2d + 2 * o);
      acc += hypotf(sx * d.x, sy * d.y);
      n += 1;
      rmax = max(rmax, max(r.x, r.y));
    }
  }
  grad_accum[g] = acc;
  seen[g] = n;
  max_radius[g] = rmax;
}

struct PlanArgs {
  const float* grad_accum;
  const int32_t* seen;
  const int32_t* max_radius;
  const float* log_scales;     // [G,3]
  const float* logit_opacity;  // [G]
  int64_t G;
  float grad_threshold, log_dense_scale, logit_min_opacity, log_max_world_scale;
  int max_screen_radius, grow;
  int32_t* action;
  int32_t* offset;
  int32_t* ws;      // [4, nb]: rows out / pruned / cloned / split of each workgroup; row 0 becomes its exclusive scan
  int32_t* totals;  // 4
  int nb;
};

__global__ __launch_bounds__(NT) void plan_action_kernel(PlanArgs a) {
  __shared__ int red[4][NT / 64];
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  int act = -1;
  if (g < a.G) {
    const float ls = fmaxf(fmaxf(a.log_scales[3 * g], a.log_scales[3 * g + 1]), a.log_scales[3 * g + 2]);
    const int n = a.seen[g];
    // the average in fp64: a correctly rounded quotient of two fp32-representable numbers, so the comparison has one answer on every
    // IEEE machine (an fp32 quotient may round ONTO the threshold from below)
    const double avg = n > 0 ? (double)a.grad_accum[g] / (double)n : 0.0;
    const bool hot = avg >= (double)a.grad_threshold;
    const bool big = ls > a.log_dense_scale;
    bool prune = a.logit_opacity[g] < a.logit_min_opacity;
    if (a.max_screen_radius > 0) prune = prune || a.max_radius[g] > a.max_screen_radius;
    prune = prune || ls > a.log_max_world_scale;  // (+inf: off)
    act = prune ? PRUNE : (hot && a.grow) ? (big ? SPLIT : CLONE) : KEEP;
    a.action[g] = act;
  }
  // the four sums of the workgroup (integers: any order gives the same number)
  int c[4] = {act < 0 ? 0 : min(act, 2), act == PRUNE, act == CLONE, act == SPLIT};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_down(c[k], o, 64);
    if (lane == 0) red[k][wave] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += red[threadIdx.x][w];
    a.ws[(int64_t)threadIdx.x * a.nb + blockIdx.x] = s;
  }
}

// one workgroup: row 0 of ws -> its exclusive scan, in chunks of NT_SUMS with a carry; rows 1 .. 3 -> their sums
__global__ __launch_bounds__(NT_SUMS) void plan_sums_kernel(int32_t* ws, int nb, int32_t* totals) {
  __shared__ int wsum[NT_SUMS / 64];
  int carry = 0, extra[3] = {0, 0, 0};
  for (int base = 0; base < nb; base += NT_SUMS) {
    const int i = base + (int)threadIdx.x;
    const int v = i < nb ? ws[i] : 0;
    int total;
    const int inc = block_scan<NT_SUMS / 64>(v, wsum, total);
    if (i < nb) {
      ws[i] = carry + inc - v;
#pragma unroll
      for (int k = 0; k < 3; ++k) extra[k] += ws[(int64_t)(k + 1) * nb + i];
    }
    carry += total;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int total;
    block_scan<NT_SUMS / 64>(extra[k], wsum, total);
    extra[k] = total;
  }
  if (threadIdx.x == 0) {
    totals[0] = carry;
    totals[1] = extra[0];
    totals[2] = extra[1];
    totals[3] = extra[2];
  }
}

__global__ __launch_bounds__(NT) void plan_offset_kernel(const int32_t* __restrict__ action, int64_t G, const int32_t* __restrict__ ws,
                                                         int32_t* __restrict__ offset) {
  __shared__ int wsum[NT / 64];
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int cnt = g < G ? min(action[g], 2) : 0;
  int total;
  const int inc = block_scan<NT / 64>(cnt, wsum, total);
  if (g < G) offset[g] = ws[blockIdx.x] + inc - cnt;
}

struct ApplyArgs {
  const float* src;
  const float* m1;  // exp_avg, exp_avg_sq of the source rows, or null (a frozen field)
  const float* m2;
  float* dst;
  float* dst_m1;
  float* dst_m2;
  const int32_t* action;
  const int32_t* offset;
  const float* quats_xyzw;  // MEANS: [G,4] raw
  const float* log_scales;  // MEANS: [G,3]
  const float* noise;       // MEANS: [G,2,3]
  uint32_t r, n;            // row width, G * r
};

enum { COPY = 0, MEANS = 1, LOG_SCALES = 2 };

template <int MODE>
__global__ __launch_bounds__(NT) void apply_kernel(ApplyArgs a) {
  const uint32_t t = blockIdx.x * (uint32_t)NT + threadIdx.x;
  if (t >= a.n) return;
  const uint32_t g = t / a.r, e = t - g * a.r;
  const int act = a.action[g];
  if (act == PRUNE) return;
  const int64_t o = (int64_t)a.offset[g] * a.r + e;
  const float v = a.src[t];
  const bool mom = a.m1 != nullptr;
  if (act != SPLIT || MODE == COPY) {
    a.dst[o] = v;
    if (mom) {
      const bool carry = act != SPLIT;
      a.dst_m1[o] = carry ? a.m1[t] : 0.f;
      a.dst_m2[o] = carry ? a.m2[t] : 0.f;
    }
    if (act != KEEP) {
      a.dst[o + a.r] = v;
      if (mom) a.dst_m1[o + a.r] = a.dst_m2[o + a.r] = 0.f;
    }
    return;
  }
  float child[2] = {v, v};
  if (MODE == LOG_SCALES) child[0] = child[1] = v - LOG_SPLIT;
  if (MODE == MEANS) {
    // row e of R(q / |q|), the quaternion stored (x, y, z, w)
    const float4 q = *(const float4*)(a.quats_xyzw + 4 * (int64_t)g);
    float R[9];
    quat_rotation(q.w, q.x, q.y, q.z, R);
    const float R0 = e == 0 ? R[0] : e == 1 ? R[3] : R[6], R1 = e == 0 ? R[1] : e == 1 ? R[4] : R[7], R2 = e == 0 ? R[2] : e == 1 ? R[5] : R[8];
    const float* ls = a.log_scales + 3 * (int64_t)g;
    const float s0 = expf(ls[0]), s1 = expf(ls[1]), s2 = expf(ls[2]);
    const float* zn = a.noise + 6 * (int64_t)g;
#pragma unroll
    for (int c = 0; c < 2; ++c) child[c] = v + (R0 * (s0 * zn[3 * c]) + R1 * (s1 * zn[3 * c + 1]) + R2 * (s2 * zn[3 * c + 2]));
  }
  a.dst[o] = child[0];
  a.dst[o + a.r] = child[1];
  if (mom) a.dst_m1[o] = a.dst_m2[o] = a.dst_m1[o + a.r] = a.dst_m2[o + a.r] = 0.f;
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)cdiv64(n, NT)); }

}  // namespace

extern "C" int siu3r_density_accumulate(const float* g_mean2d, const int32_t* radii, int V, int64_t G, float sx, float sy, float* grad_accum, int32_t* seen,
                                        int32_t* max_radius, void* stream) {
  SIU3R_CHECK(V > 0 && G >= 0, "density_accumulate: bad sizes V = %d, G = %lld", V, (long long)G);
  SIU3R_CHECK(G == 0 || (g_mean2d && radii && grad_accum && seen && max_radius), "density_accumulate: null pointer");
  SIU3R_CHECK(G <= (int64_t)0x7fffffff * NT / 2, "density_accumulate: %lld Gaussians exceed one launch", (long long)G);
  SIU3R_CHECK((((uintptr_t)g_mean2d | (uintptr_t)radii) & 7) == 0, "density_accumulate: g_mean2d and radii must be 8-byte aligned");
  if (G > 0)
    hipLaunchKernelGGL(accumulate_kernel, grid_of(G), dim3(NT), 0, (hipStream_t)stream, g_mean2d, radii, V, G, sx, sy, grad_accum, seen, max_radius);
  SIU3R_LAUNCH_CHECK("siu3r_density_accumulate");
  return 0;
}

extern "C" int64_t siu3r_density_plan_ws(int64_t G) { return G <= 0 ? 0 : 4 * cdiv64(G, NT); }

extern "C" int siu3r_density_plan(const float* grad_accum, const int32_t* seen, const int32_t* max_radius, const float* log_scales, const float* logit_opacity,
                                  int64_t G, float grad_threshold, float log_dense_scale, float logit_min_opacity, int max_screen_radius,
                                  float log_max_world_scale, int grow, int32_t* action, int32_t* offset, int32_t* ws, int32_t* totals, void* stream) {
  SIU3R_CHECK(G > 0, "density_plan: no Gaussians (G = %lld)", (long long)G);
  SIU3R_CHECK(G <= (1ll << 30), "density_plan: %lld Gaussians: the output rows (up to 2 G) must fit 32-bit offsets", (long long)G);
  SIU3R_CHECK(grad_accum && seen && max_radius && log_scales && logit_opacity && action && offset && ws && totals, "density_plan: null pointer");
  PlanArgs a;
  a.grad_accum = grad_accum, a.seen = seen, a.max_radius = max_radius, a.log_scales = log_scales, a.logit_opacity = logit_opacity;
  a.G = G;
  a.grad_threshold = grad_threshold, a.log_dense_scale = log_dense_scale, a.logit_min_opacity = logit_min_opacity;
  a.log_max_world_scale = log_max_world_scale;
  a.max_screen_radius = max_screen_radius, a.grow = grow != 0;
  a.action = action, a.offset = offset, a.ws = ws, a.totals = totals;
  a.nb = (int)cdiv64(G, NT);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(plan_action_kernel, dim3(a.nb), dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_density_plan (actions)");
  hipLaunchKernelGGL(plan_sums_kernel, dim3(1), dim3(NT_SUMS), 0, s, ws, a.nb, totals);
  SIU3R_LAUNCH_CHECK("siu3r_density_plan (workgroup sums)");
  hipLaunchKernelGGL(plan_offset_kernel, dim3(a.nb), dim3(NT), 0, s, (const int32_t*)action, G, (const int32_t*)ws, offset);
  SIU3R_LAUNCH_CHECK("siu3r_density_plan (offsets)");
  return 0;
}

extern "C" int siu3r_density_apply(int mode, const float* src, const float* m1, const float* m2, int r, int64_t G, const int32_t* action,
                                   const int32_t* offset, const float* quats_xyzw, const float* log_scales, const float* noise, float* dst, float* dst_m1,
                                   float* dst_m2, void* stream) {
  SIU3R_CHECK(mode == COPY || mode == MEANS || mode == LOG_SCALES, "density_apply: bad mode %d", mode);
  SIU3R_CHECK(G > 0 && r > 0, "density_apply: bad sizes G = %lld, r = %d", (long long)G, r);
  SIU3R_CHECK(G * r <= 0x7fffffffll, "density_apply: %lld x %d elements exceed one launch (32-bit element index)", (long long)G, r);
  SIU3R_CHECK(src && dst && action && offset, "density_apply: null pointer");
  SIU3R_CHECK((m1 != nullptr) == (m2 != nullptr), "density_apply: pass both Adam moments or neither");
  SIU3R_CHECK(!m1 || (dst_m1 && dst_m2), "density_apply: moments without an output");
  SIU3R_CHECK(mode == COPY || r == 3, "density_apply: means and log-scales have 3 columns, got %d", r);
  SIU3R_CHECK(mode != MEANS || (quats_xyzw && log_scales && noise && ((uintptr_t)quats_xyzw & 15) == 0),
              "density_apply: the means need quaternions (16-byte aligned), log-scales and noise");
  ApplyArgs a;
  a.src = src, a.m1 = m1, a.m2 = m2, a.dst = dst, a.dst_m1 = dst_m1, a.dst_m2 = dst_m2;
  a.action = action, a.offset = offset, a.quats_xyzw = quats_xyzw, a.log_scales = log_scales, a.noise = noise;
  a.r = (uint32_t)r, a.n = (uint32_t)(G * r);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = grid_of(G * r);
  if (mode == COPY)
    hipLaunchKernelGGL(apply_kernel<COPY>, grid, dim3(NT), 0, s, a);
  else if (mode == MEANS)
    hipLaunchKernelGGL(apply_kernel<MEANS>, grid, dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(apply_kernel<LOG_SCALES>, grid, dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_density_apply");
  return 0;
}
