// MCMC densification of splat refinement (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo"):
// a fixed budget of rows, dead Gaussians RELOCATED onto live ones, growth by a fixed share per event, noise on the means every iteration.
//
//   weights     w[g] = rint(sigmoid(a[g]) 2^24) as an integer (sigmoid in fp64), dead[g] = a[g] <= logit_min_opacity.  Everything that follows
//               is integer arithmetic on w: the draws are a pure function of (w, random words), the same on every machine.
//   scan        the inclusive scan of w in uint64 and the order-preserving compaction of the dead rows, in the three launches of
//               density.hip's plan: scan_sums_kernel (per-workgroup sums) -> scan_carry_kernel (ONE workgroup: exclusive scan of the sums in
//               chunks of NT_SUMS with a carry) -> scan_offset_kernel (scan inside the workgroup + its base).
//   sample      draw j: t = (rbits[j] * total) >> 32 (an 86-bit product, split), the smallest g with cum[g] > t by bisection; count[g] by
//               integer atomics.
//   relocate    the opacity / scale correction of a row drawn count[g] times, the whole row in fp64, one rounding per output.
//   copy        field[dst[j], :] = field[src[j], :], lanes along the row elements; both rows of both Adam moments become zero.
//   noise       means[g] += Sigma_g (noise[g] * gate(o_g) * scaler), fp32.
//   regularize  the gradients of lambda_o mean(o) and lambda_s mean(exp(s)), and both values by a fixed-order reduction.
// No kernel holds a float atomic, none allocates or synchronises with the host; two calls on equal inputs give equal bits.
#include "block_reduce.h"
#include "gaussian_shared.h"

namespace {

constexpr int NT = 256;  // threads per workgroup of every kernel but the scan of the workgroup sums
constexpr int NT_SUMS = 1024;
constexpr int N_MAX = 51;               // gsplat's binomial table: a row drawn more than 50 times is corrected as if drawn 50 times
constexpr double W_ONE = 16777216.0;    // 2^24: the weight of opacity 1
constexpr double O_MAX = 1.0 - 1.1920929e-07;

__device__ inline double sigmoid64(float a) { return 1.0 / (1.0 + exp(-(double)a)); }
__device__ inline float sigmoid32(float a) { return 1.0f / (1.0f + expf(-a)); }

__global__ __launch_bounds__(NT) void weights_kernel(const float* __restrict__ a, int64_t G, float logit_min, int relocate, uint32_t* __restrict__ w,
                                                     uint8_t* __restrict__ dead) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= G) return;
  const float x = a[g];
  const bool d = x <= logit_min;
  const double o = sigmoid64(x);
  const uint32_t v = o == o ? (uint32_t)rint(o * W_ONE) : 0u;  // (a NaN opacity is never drawn)
  w[g] = relocate && d ? 0u : v;
  dead[g] = d;
}

typedef unsigned long long u64;

// `dead` may be null (growth draws from every row and needs no list): the int32 half of the scan is then skipped
__global__ __launch_bounds__(NT) void scan_sums_kernel(const uint32_t* __restrict__ w, const uint8_t* __restrict__ dead, int64_t G, u64* __restrict__ wsums,
                                                       int32_t* __restrict__ dsums) {
  __shared__ u64 red64[NT / 64];
  __shared__ int red32[NT / 64];
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  u64 total;
  block_scan<NT / 64>(g < G ? (u64)w[g] : 0ull, red64, total);
  if (threadIdx.x == 0) wsums[blockIdx.x] = total;
  if (dead) {
    int n;
    block_scan<NT / 64>(g < G && dead[g] ? 1 : 0, red32, n);
    if (threadIdx.x == 0) dsums[blockIdx.x] = n;
  }
}

// one workgroup: both arrays of workgroup sums -> their exclusive scans, in chunks of NT_SUMS with a carry
__global__ __launch_bounds__(NT_SUMS) void scan_carry_kernel(u64* wsums, int32_t* dsums, int nb, int has_dead, int32_t* n_dead) {
  __shared__ u64 red64[NT_SUMS / 64];
  __shared__ int red32[NT_SUMS / 64];
  u64 carry = 0;
  int dcarry = 0;
  for (int base = 0; base < nb; base += NT_SUMS) {
    const int i = base + (int)threadIdx.x;
    const u64 v = i < nb ? wsums[i] : 0ull;
    u64 total;
    const u64 inc = block_scan<NT_SUMS / 64>(v, red64, total);
    if (i < nb) wsums[i] = carry + inc - v;
    carry += total;
    if (has_dead) {
      const int d = i < nb ? dsums[i] : 0;
      int n;
      const int dinc = block_scan<NT_SUMS / 64>(d, red32, n);
      if (i < nb) dsums[i] = dcarry + dinc - d;
      dcarry += n;
    }
  }
  if (has_dead && threadIdx.x == 0) *n_dead = dcarry;
}

__global__ __launch_bounds__(NT) void scan_offset_kernel(const uint32_t* __restrict__ w, const uint8_t* __restrict__ dead, int64_t G,
                                                         const u64* __restrict__ wsums, const int32_t* __restrict__ dsums, u64* __restrict__ cum,
                                                         int32_t* __restrict__ dead_idx) {
  __shared__ u64 red64[NT / 64];
  __shared__ int red32[NT / 64];
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  u64 total;
  const u64 inc = block_scan<NT / 64>(g < G ? (u64)w[g] : 0ull, red64, total);
  if (g < G) cum[g] = wsums[blockIdx.x] + inc;
  if (dead) {
    const int d = g < G && dead[g] ? 1 : 0;
    int n;
    const int dinc = block_scan<NT / 64>(d, red32, n);
    if (d) dead_idx[dsums[blockIdx.x] + dinc - 1] = (int32_t)g;  // (at most G dead rows: inside dead_idx [G])
  }
}

__global__ __launch_bounds__(NT) void sample_kernel(const u64* __restrict__ cum, int64_t G, const int64_t* __restrict__ rbits, int64_t n,
                                                    int32_t* __restrict__ sampled, int32_t* __restrict__ count) {
  const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const u64 total = cum[G - 1];
  int64_t lo = 0;
  if (total > 0) {
    // t = (r * total) >> 32 with r < 2^32, total < 2^54: r * hi(total) < 2^54 and r * lo(total) < 2^64, both exact
    const u64 r = (u64)rbits[j] & 0xffffffffull;
    const u64 t = r * (total >> 32) + ((r * (total & 0xffffffffull)) >> 32);
    int64_t hi = G - 1;  // cum[hi] = total > t: the answer lies in [lo, hi]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cum[mid] > t) hi = mid;
      else lo = mid + 1;
    }
  }
  sampled[j] = (int32_t)lo;
  atomicAdd(&count[lo], 1);
}

__global__ __launch_bounds__(NT) void relocate_kernel(float* __restrict__ log_scales, float* __restrict__ logit_opacity, const int32_t* __restrict__ count,
                                                      int64_t G, double min_opacity) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= G) return;
  const int c = count[g];
  if (c <= 0) return;
  const int N = min(c, N_MAX - 1) + 1;
  const double o = sigmoid64(logit_opacity[g]);
  const double o_new = 1.0 - pow(1.0 - o, 1.0 / (double)N);
  // denom = sum_{k < N} C(N, k + 1) (-1)^k o_new^(k + 1) / sqrt(k + 1): the double sum of the rule with its inner index summed by the
  // hockey-stick identity.  C(N, k + 2) = C(N, k + 1) (N - k - 1) / (k + 2) stays exact: the product is below 2^53 up to N = 51.
  double denom = 0.0, binom = (double)N, power = o_new, sign = 1.0;
  for (int k = 0; k < N; ++k) {
    denom += sign * binom * power / sqrt((double)(k + 1));
    binom = binom * (double)(N - k - 1) / (double)(k + 2);
    power *= o_new;
    sign = -sign;
  }
  const double shift = log(o / denom);
  float* s = log_scales + 3 * g;
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = (float)((double)s[k] + shift);
  const double oc = fmin(fmax(o_new, min_opacity), O_MAX);  // the clamp comes after denom, as in gsplat
  logit_opacity[g] = (float)log(oc / (1.0 - oc));
}

struct CopyArgs {
  float* field;
  float* m1;  // exp_avg, exp_avg_sq, or null (a frozen field)
  float* m2;
  const int32_t* src;
  const int32_t* dst;  // null: dst[j] = G0 + j
  uint32_t r, total;   // row width, n * r
  int64_t rows, G0;
};

__global__ __launch_bounds__(NT) void copy_rows_kernel(CopyArgs a) {
  const uint32_t t = blockIdx.x * (uint32_t)NT + threadIdx.x;
  if (t >= a.total) return;
  const uint32_t j = t / a.r, e = t - j * a.r;
  const int64_t s = a.src[j], d = a.dst ? (int64_t)a.dst[j] : a.G0 + j;
  if (s < 0 || s >= a.rows || d < 0 || d >= a.rows) return;  // (an index outside the field is not followed)
  const int64_t so = s * a.r + e, dd = d * a.r + e;
  a.field[dd] = a.field[so];
  if (a.m1) a.m1[so] = a.m1[dd] = a.m2[so] = a.m2[dd] = 0.f;
}

__global__ __launch_bounds__(NT) void noise_kernel(float* __restrict__ means, const float* __restrict__ log_scales, const float* __restrict__ quats_xyzw,
                                                   const float* __restrict__ logit_opacity, const float* __restrict__ noise, int64_t G, float gate_opacity,
                                                   float scaler) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= G) return;
  const float o = sigmoid32(logit_opacity[g]);
  const float gate = 1.0f / (1.0f + expf(-100.0f * (gate_opacity - o)));
  const float k = gate * scaler;
  const float* zn = noise + 3 * g;
  const float v0 = zn[0] * k, v1 = zn[1] * k, v2 = zn[2] * k;
  // R(q / |q|), the quaternion stored (x, y, z, w)
  const float4 q = *(const float4*)(quats_xyzw + 4 * g);
  float R[9];
  quat_rotation(q.w, q.x, q.y, q.z, R);
  const float R00 = R[0], R01 = R[1], R02 = R[2], R10 = R[3], R11 = R[4], R12 = R[5], R20 = R[6], R21 = R[7], R22 = R[8];
  const float* ls = log_scales + 3 * g;
  // Sigma v = R (exp(2 s) o (R^T v))
  const float u0 = expf(2.0f * ls[0]) * (R00 * v0 + R10 * v1 + R20 * v2);
  const float u1 = expf(2.0f * ls[1]) * (R01 * v0 + R11 * v1 + R21 * v2);
  const float u2 = expf(2.0f * ls[2]) * (R02 * v0 + R12 * v1 + R22 * v2);
  float* m = means + 3 * g;
  m[0] += R00 * u0 + R01 * u1 + R02 * u2;
  m[1] += R10 * u0 + R11 * u1 + R12 * u2;
  m[2] += R20 * u0 + R21 * u1 + R22 * u2;
}

__global__ __launch_bounds__(NT) void regularize_kernel(const float* __restrict__ logit_opacity, const float* __restrict__ log_scales, int64_t G, float c_o,
                                                        float c_s, float* __restrict__ grad_opacity, float* __restrict__ grad_scales,
                                                        double* __restrict__ partials) {
  __shared__ double red[2 * 4];
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (g < G) {
    const float o = sigmoid32(logit_opacity[g]);
    if (grad_opacity) grad_opacity[g] += c_o * (o * (1.0f - o));
    const float* s = log_scales + 3 * g;
    const float e0 = expf(s[0]), e1 = expf(s[1]), e2 = expf(s[2]);
    if (grad_scales) {
      float* gs = grad_scales + 3 * g;
      gs[0] += c_s * e0;
      gs[1] += c_s * e1;
      gs[2] += c_s * e2;
    }
    v[0] = (double)o;
    v[1] = (double)e0 + (double)e1 + (double)e2;
  }
  block_reduce<Reduce::Sum, 2>(v, red);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = v[0];
    partials[2 * (int64_t)blockIdx.x + 1] = v[1];
  }
}

// one workgroup: the partial sums in index order (thread t takes t, t + NT, ...), then the fixed-order reduction
__global__ __launch_bounds__(NT) void regularize_sum_kernel(const double* __restrict__ partials, int nb, double k_o, double k_s, float* __restrict__ value) {
  __shared__ double red[2 * 4];
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nb; i += NT) {
    v[0] += partials[2 * (int64_t)i];
    v[1] += partials[2 * (int64_t)i + 1];
  }
  block_reduce<Reduce::Sum, 2>(v, red);
  if (threadIdx.x == 0) {
    value[0] = (float)(k_o * v[0]);
    value[1] = (float)(k_s * v[1]);
  }
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)cdiv64(n, NT)); }
constexpr int64_t G_MAX = 1ll << 30;

}  // namespace

extern "C" int64_t siu3r_mcmc_ws(int64_t G) { return G <= 0 ? 0 : 16 * cdiv64(G, NT); }

extern "C" int siu3r_mcmc_weights(const float* logit_opacity, int64_t G, float logit_min_opacity, int relocate, uint32_t* w, uint8_t* dead, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_weights: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(logit_opacity && w && dead, "mcmc_weights: null pointer");
  hipLaunchKernelGGL(weights_kernel, grid_of(G), dim3(NT), 0, (hipStream_t)stream, logit_opacity, G, logit_min_opacity, relocate != 0, w, dead);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_weights");
  return 0;
}

extern "C" int siu3r_mcmc_scan(const uint32_t* w, const uint8_t* dead, int64_t G, uint64_t* cum, int32_t* dead_idx, int32_t* n_dead, void* ws, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_scan: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(w && cum && ws, "mcmc_scan: null pointer");
  SIU3R_CHECK(!dead || (dead_idx && n_dead), "mcmc_scan: a dead mask without dead_idx and n_dead");
  SIU3R_CHECK((((uintptr_t)ws | (uintptr_t)cum) & 7) == 0, "mcmc_scan: ws and cum must be 8-byte aligned");
  const int nb = (int)cdiv64(G, NT);
  u64* wsums = (u64*)ws;
  int32_t* dsums = (int32_t*)(wsums + nb);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(NT), 0, s, w, dead, G, wsums, dsums);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_scan (workgroup sums)");
  hipLaunchKernelGGL(scan_carry_kernel, dim3(1), dim3(NT_SUMS), 0, s, wsums, dsums, nb, dead != nullptr, n_dead);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_scan (carry)");
  hipLaunchKernelGGL(scan_offset_kernel, dim3(nb), dim3(NT), 0, s, w, dead, G, (const u64*)wsums, (const int32_t*)dsums, (u64*)cum, dead_idx);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_scan (offsets)");
  return 0;
}

extern "C" int siu3r_mcmc_sample(const uint64_t* cum, int64_t G, const int64_t* rbits, int64_t n, int32_t* sampled, int32_t* count, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_sample: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(n >= 0 && n <= G_MAX * 4, "mcmc_sample: n = %lld draws must lie in 0 .. 2^32", (long long)n);
  SIU3R_CHECK(cum && count && (n == 0 || (rbits && sampled)), "mcmc_sample: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(count, 0, (size_t)G * sizeof(int32_t), s);
  SIU3R_CHECK(e == hipSuccess, "mcmc_sample: clearing the counts failed: %s", hipGetErrorString(e));
  if (n > 0) hipLaunchKernelGGL(sample_kernel, grid_of(n), dim3(NT), 0, s, (const u64*)cum, G, rbits, n, sampled, count);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_sample");
  return 0;
}

extern "C" int siu3r_mcmc_relocate(float* log_scales, float* logit_opacity, const int32_t* count, int64_t G, double min_opacity, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_relocate: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(log_scales && logit_opacity && count, "mcmc_relocate: null pointer");
  SIU3R_CHECK(min_opacity > 0.0 && min_opacity < 1.0, "mcmc_relocate: min_opacity = %g must lie inside (0, 1)", min_opacity);
  hipLaunchKernelGGL(relocate_kernel, grid_of(G), dim3(NT), 0, (hipStream_t)stream, log_scales, logit_opacity, count, G, min_opacity);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_relocate");
  return 0;
}

extern "C" int siu3r_mcmc_copy_rows(float* field, float* m1, float* m2, int r, int64_t rows, const int32_t* src, const int32_t* dst, int64_t G0, int64_t n,
                                    void* stream) {
  SIU3R_CHECK(n >= 0, "mcmc_copy_rows: n = %lld is negative", (long long)n);
  SIU3R_CHECK(r > 0 && rows > 0 && rows <= 2 * G_MAX, "mcmc_copy_rows: bad sizes rows = %lld, r = %d", (long long)rows, r);
  SIU3R_CHECK(field && src, "mcmc_copy_rows: null pointer");
  SIU3R_CHECK((m1 != nullptr) == (m2 != nullptr), "mcmc_copy_rows: pass both Adam moments or neither");
  SIU3R_CHECK(dst || (G0 >= 0 && G0 + n <= rows), "mcmc_copy_rows: rows %lld .. %lld lie outside the field's %lld", (long long)G0, (long long)(G0 + n), (long long)rows);
  SIU3R_CHECK(n * r <= 0x7fffffffll, "mcmc_copy_rows: %lld x %d elements exceed one launch (32-bit element index)", (long long)n, r);
  if (n == 0) return 0;
  CopyArgs a;
  a.field = field, a.m1 = m1, a.m2 = m2, a.src = src, a.dst = dst;
  a.r = (uint32_t)r, a.total = (uint32_t)(n * r);
  a.rows = rows, a.G0 = G0;
  hipLaunchKernelGGL(copy_rows_kernel, grid_of(n * r), dim3(NT), 0, (hipStream_t)stream, a);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_copy_rows");
  return 0;
}

extern "C" int siu3r_mcmc_noise(float* means, const float* log_scales, const float* quats_xyzw, const float* logit_opacity, const float* noise, int64_t G,
                                float gate_opacity, float scaler, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_noise: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(means && log_scales && quats_xyzw && logit_opacity && noise, "mcmc_noise: null pointer");
  SIU3R_CHECK(((uintptr_t)quats_xyzw & 15) == 0, "mcmc_noise: the quaternions must be 16-byte aligned");
  hipLaunchKernelGGL(noise_kernel, grid_of(G), dim3(NT), 0, (hipStream_t)stream, means, log_scales, quats_xyzw, logit_opacity, noise, G, gate_opacity, scaler);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_noise");
  return 0;
}

extern "C" int siu3r_mcmc_regularize(const float* logit_opacity, const float* log_scales, int64_t G, float lambda_o, float lambda_s, float* grad_opacity,
                                     float* grad_scales, void* ws, float* value, void* stream) {
  SIU3R_CHECK(G > 0 && G <= G_MAX, "mcmc_regularize: G = %lld must lie in 1 .. 2^30", (long long)G);
  SIU3R_CHECK(logit_opacity && log_scales && ws && value, "mcmc_regularize: null pointer");
  SIU3R_CHECK(((uintptr_t)ws & 7) == 0, "mcmc_regularize: ws must be 8-byte aligned");
  const int nb = (int)cdiv64(G, NT);
  const float c_o = (float)((double)lambda_o / (double)G), c_s = (float)((double)lambda_s / (3.0 * (double)G));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(regularize_kernel, dim3(nb), dim3(NT), 0, s, logit_opacity, log_scales, G, c_o, c_s, grad_opacity, grad_scales, (double*)ws);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_regularize");
  hipLaunchKernelGGL(regularize_sum_kernel, dim3(1), dim3(NT), 0, s, (const double*)ws, nb, (double)lambda_o / (double)G, (double)lambda_s / (3.0 * (double)G),
                     value);
  SIU3R_LAUNCH_CHECK("siu3r_mcmc_regularize (sum)");
  return 0;
}
