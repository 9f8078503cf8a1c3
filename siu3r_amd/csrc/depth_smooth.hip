// Instance-aware depth smoothness of splat refinement: value AND gradient w.r.t. the K2 render's depth (D = sum w z)
// and opacity (O = sum w) maps, fp32 [V,H,W], contiguous, gated by an int32 segment map of the same shape (any negative id: void; no map:
// one segment, nothing void).
//
// Per pixel, in fp64 (an upcast of fp32 is exact):
//   space 0 (render):    x = D,      usable iff D is finite
//   space 1 (expected):  x = D / O,  usable iff O > min_opacity, D > 0 and both are finite;  dx/dD = 1 / O,  dx/dO = -D / O^2
// Terms along x (along y: the same with the axes swapped), owned by ONE pixel each:
//   order 1:  t = x[j+1] - x[j],             owner j (the left / top pixel), positions j = 0 .. W-2
//   order 2:  t = x[j-1] - 2 x[j] + x[j+1],  owner j (the centre),           positions j = 1 .. W-2
// A term is active iff all its pixels are usable, none is void and all carry the same segment id.  loss = Sx / n_x + Sy / n_y with
// S = sum |t| over the active terms and n = the number of POSITIONS of the axis (host-known: V H (W - order), V (H - order) W; an axis
// without a position adds 0), so the gradient is complete in one pass: d loss / dx_p = sum over the active terms holding p of
// c sign(t) / n_axis, c = -1, +1 (order 1) or 1, -2, 1 (order 2), sign(0) = 0.  The sum of c sign(t) over an axis is a small integer.
//
// Work split: a workgroup (256 threads) owns a 64 x 16 pixel tile of ONE view; a thread owns 4 consecutive pixels of a row.  The tile is
// staged in LDS as x (double) and the segment id (int) with a halo of `order` pixels on every side; an unusable pixel and a pixel outside
// the image are staged as void, so one chain of id comparisons gates a term.  Interior rows are read and the gradients written with
// 16-byte accesses where every plane's base and W allow it (one decision per workgroup), else with scalar accesses; the halo is read with
// scalar accesses.  Every interior pixel evaluates the 2 (order 1) or 3 (order 2) terms per axis it takes part in from LDS, adds the one
// it owns to the workgroup's sums and writes its own gradient: a gather, no atomics.  The workgroup reduces by the fixed tree of
// block_reduce.h and writes one record of REC doubles (Sx, Sy, active x, active y: counts up to 1,024, exact); one workgroup then adds
// the records of each view in a fixed order.  Two calls give the same bits.
#include "block_reduce.h"

namespace {

constexpr int NT = 256;  // threads per workgroup
constexpr int TW = 64;   // tile width
constexpr int TH = 16;   // tile height
constexpr int PX = 4;    // pixels per thread, consecutive in a row (TW / PX threads per row, TH rows)
constexpr int REC = 4;   // doubles per record: Sx, Sy, active terms along x, along y
constexpr float FMAX = 3.402823466e+38f;
static_assert(TW / PX * TH == NT, "one thread per 4 pixels of the tile");

struct SmoothArgs {
  const float* depth;
  const float* opacity;     // or null (space 0)
  const int32_t* segments;  // or null
  float* g_depth;           // or null: value only
  float* g_opacity;         // or null (space 0, or value only)
  double* partials;         // [V, tiles_y, tiles_x, REC]
  int H, W, expected;
  float min_opacity;
  double inv_nx, inv_ny;    // 1 / n_axis, 0 for an axis without a position
};

struct Staged {
  double x;
  int seg;
};

// what LDS holds of a pixel: x and its segment id, void (-1) for an unusable pixel
__device__ inline Staged stage(const SmoothArgs& a, float d, float o, int s) {
  const bool ok = a.expected ? (o > a.min_opacity && o <= FMAX && d > 0.f && d <= FMAX) : (fabsf(d) <= FMAX);  // (false for a NaN)
  Staged r;
  r.seg = ok && s >= 0 ? s : -1;
  r.x = r.seg < 0 ? 0.0 : (a.expected ? (double)d / (double)o : (double)d);
  return r;
}

struct Term {
  bool active;
  int sign;
  double mag;
};

// the term owned by staged cell i along the axis of stride st
template <int ORDER>
__device__ inline Term term_at(const double* xs, const int* ss, int i, int st) {
  const int s0 = ss[i];
  Term r;
  double t;
  if (ORDER == 1) {
    r.active = s0 >= 0 && ss[i + st] == s0;
    t = xs[i + st] - xs[i];
  } else {
    r.active = s0 >= 0 && ss[i - st] == s0 && ss[i + st] == s0;
    t = (xs[i - st] - 2.0 * xs[i]) + xs[i + st];
  }
  r.sign = r.active ? (t > 0.0 ? 1 : (t < 0.0 ? -1 : 0)) : 0;
  r.mag = r.active ? fabs(t) : 0.0;
  return r;
}

template <int ORDER, bool GRAD>
__global__ __launch_bounds__(NT) void depth_smooth_kernel(SmoothArgs a) {
  constexpr int HALO = ORDER, SW = TW + 2 * HALO, SH = TH + 2 * HALO;
  __shared__ double xs[SH * SW];
  __shared__ int ss[SH * SW];
  __shared__ double red[REC * 4];
  const int H = a.H, W = a.W;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  const float* dp = a.depth + base;
  const float* op = a.opacity ? a.opacity + base : nullptr;
  const int32_t* sp = a.segments ? a.segments + base : nullptr;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int r = threadIdx.x / (TW / PX), c = threadIdx.x % (TW / PX) * PX;  // the thread's pixels: tile row r, columns c .. c + 3
  const int gy = y0 + r, gx = x0 + c;
  // one decision per workgroup: with W a multiple of 4 every row starts as aligned as the plane, and the tile's columns start at multiples of 64
  const bool vec = (W & 3) == 0 && aligned16(dp) && (!op || aligned16(op)) && (!sp || aligned16(sp)) &&
                   (!GRAD || (aligned16(a.g_depth + base) && (!a.g_opacity || aligned16(a.g_opacity + base))));
  float d[PX], o[PX];
  int s[PX];
  const bool row_in = gy < H;
  const int64_t off = (int64_t)gy * W + gx;  // (used only where the pixel is inside the image)
  if (vec && row_in && gx + PX <= W) {
    const float4 q = *reinterpret_cast<const float4*>(dp + off);
    d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
    if (op) {
      const float4 p = *reinterpret_cast<const float4*>(op + off);
      o[0] = p.x, o[1] = p.y, o[2] = p.z, o[3] = p.w;
    }
    if (sp) {
      const int4 p = *reinterpret_cast<const int4*>(sp + off);
      s[0] = p.x, s[1] = p.y, s[2] = p.z, s[3] = p.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const bool in = row_in && gx + k < W;
      d[k] = in ? dp[off + k] : __builtin_nanf("");  // (outside the image: unusable in both spaces)
      if (op) o[k] = in ? op[off + k] : 0.f;
      if (sp) s[k] = in ? sp[off + k] : -1;
    }
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    if (!op) o[k] = 1.f;
    if (!sp) s[k] = 0;
    const Staged st = stage(a, d[k], o[k], s[k]);
    const int i = (r + HALO) * SW + c + HALO + k;
    xs[i] = st.x, ss[i] = st.seg;
  }
  // the halo: HALO rows above and below over the whole staged width, then HALO columns left and right of the TH interior rows
  constexpr int NROWS = 2 * HALO * SW, NHALO = NROWS + TH * 2 * HALO;
  for (int i = threadIdx.x; i < NHALO; i += NT) {
    int R, C;
    if (i < NROWS) {
      const int q = i / SW;
      R = q < HALO ? q : TH + q;
      C = i - q * SW;
    } else {
      const int j = i - NROWS, q = j / (2 * HALO), k = j - q * (2 * HALO);
      R = HALO + q;
      C = k < HALO ? k : TW + k;
    }
    const int py = y0 + R - HALO, px = x0 + C - HALO;
    Staged st;
    st.x = 0.0, st.seg = -1;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const int g = py * W + px;
      st = stage(a, dp[g], op ? op[g] : 1.f, sp ? sp[g] : 0);
    }
    xs[R * SW + C] = st.x, ss[R * SW + C] = st.seg;
  }
  __syncthreads();

  double sum[REC] = {0.0, 0.0, 0.0, 0.0};
  float gd[PX], go[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    gd[k] = go[k] = 0.f;
    const int i = (r + HALO) * SW + c + HALO + k;
    if (!(row_in && gx + k < W) || ss[i] < 0) continue;  // (a void pixel owns no active term and takes part in none)
    const Term tx = term_at<ORDER>(xs, ss, i, 1), ty = term_at<ORDER>(xs, ss, i, SW);
    sum[0] += tx.mag, sum[1] += ty.mag;
    sum[2] += tx.active ? 1.0 : 0.0, sum[3] += ty.active ? 1.0 : 0.0;
    if (GRAD) {
      int kx, ky;  // sum of c sign(t) over the terms of the axis that hold this pixel
      if (ORDER == 1) {
        kx = term_at<1>(xs, ss, i - 1, 1).sign - tx.sign;
        ky = term_at<1>(xs, ss, i - SW, SW).sign - ty.sign;
      } else {
        kx = term_at<2>(xs, ss, i - 1, 1).sign - 2 * tx.sign + term_at<2>(xs, ss, i + 1, 1).sign;
        ky = term_at<2>(xs, ss, i - SW, SW).sign - 2 * ty.sign + term_at<2>(xs, ss, i + SW, SW).sign;
      }
      const double g = (double)kx * a.inv_nx + (double)ky * a.inv_ny;
      if (g != 0.0) {  // (else +0, whatever the sign of the chain's factors)
        if (a.expected) {
          const double iO = 1.0 / (double)o[k];
          gd[k] = (float)(g * iO);
          go[k] = (float)(g * (-((double)d[k] * iO) * iO));
        } else {
          gd[k] = (float)g;
        }
      }
    }
  }
  if (GRAD && row_in) {
    if (vec && gx + PX <= W) {
      *reinterpret_cast<float4*>(a.g_depth + base + off) = make_float4(gd[0], gd[1], gd[2], gd[3]);
      if (a.g_opacity) *reinterpret_cast<float4*>(a.g_opacity + base + off) = make_float4(go[0], go[1], go[2], go[3]);
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        if (gx + k < W) {
          a.g_depth[base + off + k] = gd[k];
          if (a.g_opacity) a.g_opacity[base + off + k] = go[k];
        }
      }
    }
  }
  block_reduce<Reduce::Sum>(sum, red);
  if (threadIdx.x == 0) {
    double* rec = a.partials + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * REC;
#pragma unroll
    for (int k = 0; k < REC; ++k) rec[k] = sum[k];
  }
}

// one workgroup: per view, thread t adds the records t, t + 256, ... in that order, then the fixed tree; the views in index order.
// out = (loss, x-axis part, y-axis part, 0); per_view[v] = the view's two parts over its own positions; active[v] = its exact counts
__global__ __launch_bounds__(NT) void depth_smooth_finalize_kernel(const double* partials, int V, int tpv, double inv_nx, double inv_ny, float* out,
                                                                   float* per_view, int32_t* active) {
  __shared__ double red[REC * 4];
  double sx = 0.0, sy = 0.0;
  for (int v = 0; v < V; ++v) {
    const double* pv = partials + (int64_t)v * tpv * REC;
    double s[REC] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < tpv; i += NT) {
      const double* rec = pv + (int64_t)i * REC;
      s[0] += rec[0], s[1] += rec[1], s[2] += rec[2], s[3] += rec[3];
    }
    block_reduce<Reduce::Sum>(s, red);
    sx += s[0], sy += s[1];
    if (threadIdx.x == 0) {  // (a view's positions: 1 / V of the axis')
      per_view[v] = (float)(s[0] * inv_nx * (double)V + s[1] * inv_ny * (double)V);
      active[2 * v] = (int32_t)s[2], active[2 * v + 1] = (int32_t)s[3];
    }
  }
  if (threadIdx.x == 0) {
    const double px = sx * inv_nx, py = sy * inv_ny;
    out[0] = (float)(px + py), out[1] = (float)px, out[2] = (float)py, out[3] = 0.f;
  }
}

int tiles_x(int W) { return (W + TW - 1) / TW; }
int tiles_y(int H) { return (H + TH - 1) / TH; }

}  // namespace

extern "C" int64_t siu3r_depth_smooth_ws(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0 || V > 65535 || (int64_t)H * W > 0x7fffffff - TW * TH || tiles_y(H) > 65535) return 0;
  return (int64_t)V * tiles_y(H) * tiles_x(W) * REC * (int64_t)sizeof(double);
}

extern "C" int siu3r_depth_smooth(const float* depth, const float* opacity, const int32_t* segments, int V, int H, int W, int order, int space,
                                  float min_opacity, float* g_depth, float* g_opacity, void* ws, float* out, float* per_view, int32_t* active,
                                  void* stream) {
  SIU3R_CHECK(depth && ws && out && per_view && active, "depth_smooth: null pointer");
  SIU3R_CHECK(V > 0 && H > 0 && W > 0, "depth_smooth: empty input [%d,%d,%d]", V, H, W);
  SIU3R_CHECK((int64_t)H * W <= 0x7fffffff - TW * TH, "depth_smooth: %d x %d pixels per view exceed 32-bit indexing", H, W);
  SIU3R_CHECK(V <= 65535 && tiles_y(H) <= 65535, "depth_smooth: %d views of %d rows exceed one launch", V, H);
  SIU3R_CHECK(order == 1 || order == 2, "depth_smooth: order %d (1 or 2)", order);
  SIU3R_CHECK(space == 0 || space == 1, "depth_smooth: space %d (0 render, 1 expected)", space);
  SIU3R_CHECK(min_opacity >= 0.f && min_opacity <= FMAX, "depth_smooth: min_opacity %g must be finite and >= 0", (double)min_opacity);
  SIU3R_CHECK(space == 0 || opacity, "depth_smooth: space 1 (expected) needs the opacity map");
  SIU3R_CHECK(g_depth || !g_opacity, "depth_smooth: g_opacity without g_depth");
  SIU3R_CHECK(space == 0 || !g_depth || g_opacity, "depth_smooth: space 1 (expected) writes g_depth and g_opacity together");
  SIU3R_CHECK(((uintptr_t)ws & 7) == 0, "depth_smooth: the workspace must be 8-byte aligned");
  SmoothArgs a;
  a.depth = depth, a.opacity = space ? opacity : nullptr, a.segments = segments;
  a.g_depth = g_depth, a.g_opacity = g_opacity;
  a.partials = (double*)ws;
  a.H = H, a.W = W, a.expected = space;
  a.min_opacity = min_opacity;
  const double nx = W > order ? (double)V * H * (W - order) : 0.0, ny = H > order ? (double)V * (H - order) * W : 0.0;
  a.inv_nx = nx > 0.0 ? 1.0 / nx : 0.0;
  a.inv_ny = ny > 0.0 ? 1.0 / ny : 0.0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_x(W), (unsigned)tiles_y(H), (unsigned)V);
  if (order == 1) {
    if (g_depth)
      hipLaunchKernelGGL((depth_smooth_kernel<1, true>), grid, dim3(NT), 0, s, a);
    else
      hipLaunchKernelGGL((depth_smooth_kernel<1, false>), grid, dim3(NT), 0, s, a);
  } else {
    if (g_depth)
      hipLaunchKernelGGL((depth_smooth_kernel<2, true>), grid, dim3(NT), 0, s, a);
    else
      hipLaunchKernelGGL((depth_smooth_kernel<2, false>), grid, dim3(NT), 0, s, a);
  }
  SIU3R_LAUNCH_CHECK("siu3r_depth_smooth");
  hipLaunchKernelGGL(depth_smooth_finalize_kernel, dim3(1), dim3(NT), 0, s, (const double*)a.partials, V, tiles_y(H) * tiles_x(W), a.inv_nx, a.inv_ny, out,
                     per_view, active);
  SIU3R_LAUNCH_CHECK("siu3r_depth_smooth (final sum)");
  return 0;
}
