// Fused photometric loss of splat refinement: (1 - lambda) * L1 + lambda * (1 - SSIM), value AND gradient in one visit.
//
// SSIM is metrics.ssim with an explicit data_range: separable 11-tap Gaussian window (sigma 1.5), per channel, both local variances clamped
// at 0, the map averaged over the valid region (H - 10) x (W - 10).  One workgroup owns a 32 x 32 tile of one (view, channel) plane:
//   1. stage the tile with its halo (10 pixels with a gradient, 0 / 10 without) of pred and target in LDS;
//   2. horizontal 11-tap pass -> five window sums (p, t, pp, tp, tt) per (row, window column), of the values MINUS a per-tile constant
//      (the tile's centre pixel): variances are shift-invariant, and e_pp - mu_p^2 of the shifted values keeps its bits on smooth regions;
//   3. vertical pass -> per window the SSIM value (summed for the windows the tile owns) and the three derivative maps
//      d_mu', d_epp, d_ept of the closed form below (zero outside the valid region);
//   4. the transposed blur of the three maps (vertical, then horizontal) and grad = d_mu' + 2 p' d_epp + t' d_ept per pixel, plus the L1
//      sign; one coalesced store in pred's layout.
// With p' = p - cp, t' = t - ct the centred form  dSSIM/dp(x) = sum_w g(w, x) [ dmu_c + 2 d_epp (p(x) - mu_p(w)) + d_ept (t(x) - mu_t(w)) ]
// needs only shifted quantities: d_mu' = dmu_c - 2 d_epp mu_p' - d_ept mu_t', dmu_c = 2 mu_t A2 / (B1 B2) - 2 mu_p A1 A2 / (B1^2 B2).
// The value is deterministic: per-workgroup partial sums (fixed tree) into `partials`, then one workgroup adds them in a fixed order.
#include "block_reduce.h"

namespace {

constexpr int TILE = 32;     // output tile edge
constexpr int TAPS = 11;     // window size
constexpr int HALO = TAPS - 1;
constexpr int NT = 256;      // threads per workgroup

// exp(-(d / 1.5)^2 / 2) / sum, d = -5 .. 5 (metrics._gauss1d(11, 1.5) rounded to fp32)
__device__ constexpr float GW[TAPS] = {0.0010283801f, 0.0075987582f, 0.0360007733f, 0.1093606874f, 0.2130055428f, 0.2660117149f,
                                       0.2130055428f, 0.1093606874f, 0.0360007733f, 0.0075987582f, 0.0010283801f};

struct PhotoArgs {
  const float* pred;
  const float* target;
  float* grad;  // pred's layout, or null
  float* partials;
  int V, C, H, W;
  int64_t ps[4], ts[4];  // element strides of (view, channel, row, column)
  int tiles_x, tiles_y;
  float c1, c2;
  float w_l1, w_ssim;  // d loss / d (sum |p - t|), d loss / d (sum of the SSIM map)
  int do_l1;
};

// fixed-order sum over the workgroup (block_reduce.h): shuffle tree per wave, then the four wave sums in index order
__device__ inline float block_sum(float v, float* red) {
  float s[1] = {v};
  block_reduce<Reduce::Sum>(s, red);
  return s[0];
}

// GRAD: windows [tile - 10, tile + 32) and pixels [tile - 10, tile + 42); otherwise windows [tile, tile + 32), pixels [tile, tile + 42)
template <bool GRAD>
__global__ __launch_bounds__(NT) void photo_ssim_kernel(PhotoArgs a) {
  constexpr int WLO = GRAD ? HALO : 0;
  constexpr int NW = TILE + WLO;   // windows per axis
  constexpr int NP = NW + HALO;    // staged pixels per axis
  constexpr int SP = NP + 1;       // odd row strides: a column of rows spreads over the banks
  constexpr int SW = NW + 1;
  constexpr int SO = TILE + 1;
  constexpr int R = 7;             // outputs per thread and pass (R + 10 inputs)
  constexpr int NSEG = (NW + R - 1) / R;
  static_assert(NW * NSEG <= NT, "the vertical pass is one round");
  __shared__ float sP[NP * SP], sT[NP * SP];
  __shared__ float sA[5 * NP * SW];  // horizontal sums; later the derivative maps, their vertical blur and the tile's SSIM gradient
  __shared__ float red[4];
  float* sD = sA;                         // [3][NW][SW]
  float* sE = sA + 3 * NW * SW;           // [3][TILE][SW]
  float* sO = sE + 3 * TILE * SW;         // [TILE][SO]
  static_assert(!GRAD || 3 * NW * SW + 3 * TILE * SW + TILE * SO <= 5 * NP * SW, "the backward planes reuse the forward's");

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  b /= a.tiles_y;
  const int ch = b % a.C, view = b / a.C;
  const int y0 = ty * TILE, x0 = tx * TILE;
  const float* pp = a.pred + view * a.ps[0] + ch * a.ps[1];
  const float* tp = a.target + view * a.ts[0] + ch * a.ts[1];
  const int H = a.H, W = a.W;

  // the shift: the tile's centre pixel (inside the image)
  const int yc = min(y0 + TILE / 2, H - 1), xc = min(x0 + TILE / 2, W - 1);
  const float cp = pp[yc * a.ps[2] + xc * a.ps[3]], ct = tp[yc * a.ts[2] + xc * a.ts[3]];

  // every load of the thread is issued before the first LDS store waits for one (addresses clamped into the image, so none is conditional)
  constexpr int NLD = (NP * NP + NT - 1) / NT;
  float vp[NLD], vt[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int i = min(tid + k * NT, NP * NP - 1);
    const int y = min(max(y0 - WLO + i / NP, 0), H - 1), x = min(max(x0 - WLO + i % NP, 0), W - 1);
    vp[k] = pp[y * a.ps[2] + x * a.ps[3]];
    vt[k] = tp[y * a.ts[2] + x * a.ts[3]];
  }
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int i = tid + k * NT;
    if (i < NP * NP) {
      const int r = i / NP, c = i % NP;
      const int y = y0 - WLO + r, x = x0 - WLO + c;
      const bool in = y >= 0 && y < H && x >= 0 && x < W;  // outside the image: the shift itself (only invalid windows see it)
      sP[r * SP + c] = in ? vp[k] : cp;
      sT[r * SP + c] = in ? vt[k] : ct;
    }
  }
  __syncthreads();

  // horizontal pass: lanes run down the rows (odd stride), R window columns per thread
  for (int it = tid; it < NSEG * NP; it += NT) {
    const int row = it % NP, j0 = (it / NP) * R;
    float p[R + HALO], t[R + HALO];
#pragma unroll
    for (int k = 0; k < R + HALO; ++k) {
      const int c = min(j0 + k, NP - 1);
      p[k] = sP[row * SP + c] - cp;
      t[k] = sT[row * SP + c] - ct;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (j0 + r < NW) {
        float mp = 0.f, mt = 0.f, epp = 0.f, ept = 0.f, ett = 0.f;
#pragma unroll
        for (int m = 0; m < TAPS; ++m) {
          const float gp = GW[m] * p[r + m], gt = GW[m] * t[r + m];
          mp += gp;
          mt += gt;
          epp = fmaf(gp, p[r + m], epp);
          ept = fmaf(gp, t[r + m], ept);
          ett = fmaf(gt, t[r + m], ett);
        }
        const int o = row * SW + j0 + r;
        sA[o] = mp;
        sA[NP * SW + o] = mt;
        sA[2 * NP * SW + o] = epp;
        sA[3 * NP * SW + o] = ept;
        sA[4 * NP * SW + o] = ett;
      }
    }
  }
  __syncthreads();

  // vertical pass: lanes run along the window columns, R window rows per thread; SSIM and the derivative maps stay in registers
  float ssim_sum = 0.f;
  float dmu[R], dpp[R], dpt[R];
  const bool vert = tid < NW * NSEG;
  const int vcol = tid % NW, vi0 = (tid / NW) * R;
  if (vert) {
    float acc[5][R];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float v[R + HALO];
#pragma unroll
      for (int k = 0; k < R + HALO; ++k) v[k] = sA[q * NP * SW + min(vi0 + k, NP - 1) * SW + vcol];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < TAPS; ++m) s = fmaf(GW[m], v[r + m], s);
        acc[q][r] = s;
      }
    }
    const int wx = x0 - WLO + vcol;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = vi0 + r, wy = y0 - WLO + i;
      const bool valid = i < NW && wy >= 0 && wy <= H - TAPS && wx >= 0 && wx <= W - TAPS;
      const float mp_s = acc[0][r], mt_s = acc[1][r];
      const float mp = mp_s + cp, mt = mt_s + ct;
      const float spp_raw = acc[2][r] - mp_s * mp_s, stt_raw = acc[4][r] - mt_s * mt_s, spt = acc[3][r] - mp_s * mt_s;
      const float spp = fmaxf(spp_raw, 0.f), stt = fmaxf(stt_raw, 0.f);
      const float A1 = 2.f * mp * mt + a.c1, A2 = 2.f * spt + a.c2;
      const float B1 = mp * mp + mt * mt + a.c1, B2 = spp + stt + a.c2;
      const float iB = 1.f / (B1 * B2);
      const float s = A1 * A2 * iB;
      if (valid && i >= WLO && vcol >= WLO) ssim_sum += s;
      if (GRAD) {
        const float d_epp = spp_raw > 0.f ? -s / B2 : 0.f;
        const float d_ept = 2.f * A1 * iB;
        const float dmu_c = 2.f * mt * A2 * iB - 2.f * mp * s / B1;
        dpp[r] = valid ? d_epp : 0.f;
        dpt[r] = valid ? d_ept : 0.f;
        dmu[r] = valid ? dmu_c - 2.f * d_epp * mp_s - d_ept * mt_s : 0.f;
      }
    }
  }
  const float ssim_total = block_sum(ssim_sum, red);  // (its barriers also end every read of the horizontal sums)

  if (GRAD) {
    if (vert) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (vi0 + r < NW) {
          const int o = (vi0 + r) * SW + vcol;
          sD[o] = dmu[r];
          sD[NW * SW + o] = dpp[r];
          sD[2 * NW * SW + o] = dpt[r];
        }
      }
    }
    __syncthreads();
    // transposed blur, vertical: pixel row r of the tile collects the window rows r .. r + 10 (local), 8 rows per thread
    constexpr int RB = 8;
    for (int it = tid; it < NW * (TILE / RB); it += NT) {
      const int col = it % NW, r0 = (it / NW) * RB;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[RB + HALO];
#pragma unroll
        for (int k = 0; k < RB + HALO; ++k) v[k] = sD[q * NW * SW + (r0 + k) * SW + col];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          float s = 0.f;
#pragma unroll
          for (int m = 0; m < TAPS; ++m) s = fmaf(GW[m], v[r + m], s);
          sE[q * TILE * SW + (r0 + r) * SW + col] = s;
        }
      }
    }
    __syncthreads();
    // transposed blur, horizontal: lanes run down the rows, 4 columns per thread
    constexpr int RC = 4;
    for (int it = tid; it < TILE * (TILE / RC); it += NT) {
      const int row = it % TILE, c0 = (it / TILE) * RC;
      float o[3][RC];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[RC + HALO];
#pragma unroll
        for (int k = 0; k < RC + HALO; ++k) v[k] = sE[q * TILE * SW + row * SW + c0 + k];
#pragma unroll
        for (int c = 0; c < RC; ++c) {
          float s = 0.f;
#pragma unroll
          for (int m = 0; m < TAPS; ++m) s = fmaf(GW[m], v[c + m], s);
          o[q][c] = s;
        }
      }
#pragma unroll
      for (int c = 0; c < RC; ++c) {
        const int li = (row + WLO) * SP + c0 + c + WLO;
        const float ps_ = sP[li] - cp, ts_ = sT[li] - ct;
        sO[row * SO + c0 + c] = o[0][c] + 2.f * ps_ * o[1][c] + ts_ * o[2][c];
      }
    }
    __syncthreads();
  }

  // the tile's own pixels: L1 and the store (lanes along the columns)
  float l1 = 0.f;
  if (a.do_l1 || GRAD) {
    for (int i = tid; i < TILE * TILE; i += NT) {
      const int r = i / TILE, c = i % TILE;
      const int y = y0 + r, x = x0 + c;
      if (y < H && x < W) {
        float g = GRAD ? a.w_ssim * sO[r * SO + c] : 0.f;
        if (a.do_l1) {
          const float d = sP[(r + WLO) * SP + c + WLO] - sT[(r + WLO) * SP + c + WLO];
          l1 += fabsf(d);
          g += d > 0.f ? a.w_l1 : (d < 0.f ? -a.w_l1 : 0.f);
        }
        if (GRAD) a.grad[view * a.ps[0] + ch * a.ps[1] + y * a.ps[2] + x * a.ps[3]] = g;
      }
    }
  }
  const float l1_total = a.do_l1 ? block_sum(l1, red) : 0.f;
  if (tid == 0) {
    a.partials[2 * (int64_t)blockIdx.x] = l1_total;
    a.partials[2 * (int64_t)blockIdx.x + 1] = ssim_total;
  }
}

// lambda = 0: no window at all, one pixel per thread of the same tiling (so that `partials` has one layout)
__global__ __launch_bounds__(NT) void photo_l1_kernel(PhotoArgs a) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  b /= a.tiles_y;
  const int ch = b % a.C, view = b / a.C;
  const float* pp = a.pred + view * a.ps[0] + ch * a.ps[1];
  const float* tp = a.target + view * a.ts[0] + ch * a.ts[1];
  float l1 = 0.f;
  for (int i = tid; i < TILE * TILE; i += NT) {
    const int y = ty * TILE + i / TILE, x = tx * TILE + i % TILE;
    if (y < a.H && x < a.W) {
      const float d = pp[y * a.ps[2] + x * a.ps[3]] - tp[y * a.ts[2] + x * a.ts[3]];
      l1 += fabsf(d);
      if (a.grad) a.grad[view * a.ps[0] + ch * a.ps[1] + y * a.ps[2] + x * a.ps[3]] = d > 0.f ? a.w_l1 : (d < 0.f ? -a.w_l1 : 0.f);
    }
  }
  const float l1_total = block_sum(l1, red);
  if (tid == 0) {
    a.partials[2 * (int64_t)blockIdx.x] = l1_total;
    a.partials[2 * (int64_t)blockIdx.x + 1] = 0.f;
  }
}

// one workgroup: thread t adds partials t, t + 256, ... in that order (fp64), then a fixed tree
__global__ __launch_bounds__(NT) void photo_finalize_kernel(const float* partials, int64_t n, double inv_l1, double inv_ssim, float lambda, int do_l1,
                                                           int do_ssim, float* out) {
  __shared__ double s0[NT], s1[NT];
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += NT) {
    a0 += (double)partials[2 * i];
    a1 += (double)partials[2 * i + 1];
  }
  s0[threadIdx.x] = a0;
  s1[threadIdx.x] = a1;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s0[threadIdx.x] += s0[threadIdx.x + o];
      s1[threadIdx.x] += s1[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double l1 = s0[0] * inv_l1, ss = s1[0] * inv_ssim;
    double loss = 0.0;
    if (do_l1) loss += (1.0 - (double)lambda) * l1;
    if (do_ssim) loss += (double)lambda * (1.0 - ss);
    const float nan = __builtin_nanf("");
    out[0] = (float)loss;
    out[1] = do_l1 ? (float)l1 : nan;
    out[2] = do_ssim ? (float)ss : nan;
  }
}

}  // namespace

extern "C" int64_t siu3r_photo_loss_partials(int V, int C, int H, int W) {
  if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)V * C * ((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);
}

extern "C" int siu3r_photo_loss(const float* pred, const float* target, int V, int C, int H, int W, const int64_t* pred_strides,
                                const int64_t* target_strides, float lambda, float data_range, float* grad_pred, float* partials, float* out,
                                void* stream) {
  SIU3R_CHECK(pred && target && partials && out && pred_strides && target_strides, "photo_loss: null pointer");
  SIU3R_CHECK(V > 0 && C > 0 && H > 0 && W > 0, "photo_loss: empty input [%d,%d,%d,%d]", V, C, H, W);
  SIU3R_CHECK(lambda >= 0.f && lambda <= 1.f, "photo_loss: lambda %g outside [0, 1]", (double)lambda);
  SIU3R_CHECK(data_range > 0.f, "photo_loss: data_range %g must be positive", (double)data_range);
  const bool do_ssim = lambda != 0.f, do_l1 = lambda != 1.f;
  SIU3R_CHECK(!do_ssim || (H >= TAPS && W >= TAPS), "photo_loss: SSIM needs at least %d x %d pixels, got %d x %d", TAPS, TAPS, H, W);
  const int64_t n = siu3r_photo_loss_partials(V, C, H, W);
  SIU3R_CHECK(n <= 0x3fffffff, "photo_loss: %lld tiles exceed one launch", (long long)n);
  for (int i = 0; i < 4; ++i)
    SIU3R_CHECK(pred_strides[i] >= 0 && target_strides[i] >= 0, "photo_loss: negative strides are not supported");
  PhotoArgs a;
  a.pred = pred;
  a.target = target;
  a.grad = grad_pred;
  a.partials = partials;
  a.V = V, a.C = C, a.H = H, a.W = W;
  for (int i = 0; i < 4; ++i) a.ps[i] = pred_strides[i], a.ts[i] = target_strides[i];
  a.tiles_x = (W + TILE - 1) / TILE;
  a.tiles_y = (H + TILE - 1) / TILE;
  a.c1 = (0.01f * data_range) * (0.01f * data_range);
  a.c2 = (0.03f * data_range) * (0.03f * data_range);
  const double n_l1 = (double)V * C * H * W, n_ssim = do_ssim ? (double)V * C * (H - HALO) * (W - HALO) : 1.0;
  a.w_l1 = (float)((1.0 - (double)lambda) / n_l1);
  a.w_ssim = (float)(-(double)lambda / n_ssim);
  a.do_l1 = do_l1;
  hipStream_t s = (hipStream_t)stream;
  if (!do_ssim)
    hipLaunchKernelGGL(photo_l1_kernel, dim3((unsigned)n), dim3(NT), 0, s, a);
  else if (grad_pred)
    hipLaunchKernelGGL(photo_ssim_kernel<true>, dim3((unsigned)n), dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(photo_ssim_kernel<false>, dim3((unsigned)n), dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_photo_loss");
  hipLaunchKernelGGL(photo_finalize_kernel, dim3(1), dim3(NT), 0, s, (const float*)partials, n, 1.0 / n_l1, 1.0 / n_ssim, lambda, (int)do_l1, (int)do_ssim,
                     out);
  SIU3R_LAUNCH_CHECK("siu3r_photo_loss (final sum)");
  return 0;
}
