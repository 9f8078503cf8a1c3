// Bilateral-grid appearance correction of splat refinement: per view a low-resolution 3-D grid of 3 x 4 colour matrices,
// indexed by pixel position and by the pixel's own luminance (Wang et al., Bilateral Guided Radiance Field Processing, 2024).
//
// Conventions.  grids [V,12,L,Gh,Gw] fp32, channel 4c + k = entry (c, k).  For pixel (y, x) with colour p = (r, g, b):
//   lum = 0.299 r + 0.587 g + 0.114 b;  fx = (x + 0.5) / W * (Gw - 1);  fy = (y + 0.5) / H * (Gh - 1);  fz = clamp(lum, 0, 1) * (L - 1)
//   x0 = min(floor(fx), Gw - 2), tx = fx - x0, likewise y and z;  M = the trilinear interpolation of the 8 corner matrices as nested
//   a + t (b - a) steps, each one fma, x first, then y, then z;  out[c] = M[c,0] r + M[c,1] g + M[c,2] b + M[c,3].
// A grid that is constant along an axis is reproduced exactly along it (b - a is 0), so the identity grid returns the bits of a finite input
// (a -0 comes back as +0), as siu3r_exposure_apply does.  A NaN luminance clamps to 0 (fmaxf), so a NaN pixel stays inside the grid.
//
// Slice (forward, and the backward to the image).  Streams like camera.hip's: a workgroup (256 threads, 2 rounds of 4 consecutive pixels) owns
// 2,048 consecutive pixels of ONE view, image_io.h moves them.  Its pixels cover a few image rows, so they reach all Gw vertex columns of
// the vertex rows y0(first row) .. y0(last row) + 1.  Those rows, every level, are staged in LDS as [vertex row][vertex column][level][12]:
// a pixel then reads each of its 8 corner matrices with three 16-byte LDS reads instead of 12 floats that lie L Gh Gw apart in memory.
// SWITCH: the host bounds the vertex rows a workgroup can reach, ny = min(Gh, floor((rows - 1) (Gh - 1) / H) + 4) with rows = the image rows
// 2,048 consecutive pixels can touch; staging is used iff ny * Gw * L * 48 bytes <= 64 KB (the default grid at 512 x 512: 4 rows, 24 KB).
// Otherwise (a grid much finer than the image, a very wide grid), and in any workgroup whose own row count exceeds the host's bound, the
// corners are read from global memory.  The backward to the image adds the guidance term: dM/dz = A1 - A0, the two xy-interpolated levels the
// z step already holds, so g_in[k] = sum_c M[c,k] g[c] + lw[k] (L - 1) [0 < lum < 1] sum_c g[c] (dM/dz [c,:] . (r, g, b, 1)).
//
// Grid gradient: a GATHER.  A scatter would add 8 x 12 values per pixel into the grid with float atomics, whose order changes from run to
// run.  Instead one workgroup owns one (view, iy, ix) vertex column and walks the pixel window in which that vertex has xy weight (about
// 2H/(Gh-1) x 2W/(Gw-1) pixels; the window is bounded in fp64 with a margin and each pixel decides membership with the slice's own y0 / x0).
// A thread keeps 12 x 8 fp32 sums, indexed only by fully unrolled loops: the level weight is the branch-free hat max(0, 1 - |fz - l|), which
// equals the slice's (1 - tz, tz) on the kernel's own z0 (to one rounding at l = z0 + 1).  L > 8 walks the window once per 8 levels.  The sums
// of the 256 threads are added by the fixed fp64 tree of block_reduce.h and the workgroup writes its own 12 L values: no atomics, two calls
// give the same bits, a vertex whose window holds no pixel writes exact zeros.
//
// Total variation.  tv = (1/V) sum_v sum_axis mean((A[i+1] - A[i])^2): fp32 differences, fp64 products and sums in a fixed order (per thread
// grid-stride, the tree per workgroup, one record per workgroup, a second launch adds the records in index order).  The same pass adds
// scale * d tv / d grids into g_grids, one thread per element.
#include "image_io.h"

extern __shared__ float4 stage[];  // the staged vertices: [vertex row][vertex column][level][3]

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int ROUNDS = 2;
constexpr int CHUNK = NT * PX * ROUNDS;  // pixels per workgroup of the two streams
constexpr int LMAX = 16;                 // levels
constexpr int GMAX = 1024;               // vertices per axis
constexpr int LB = 8;                    // levels per walk of the grid gradient
constexpr int PF = 4;                    // pixels a thread of the grid gradient loads before it adds them
constexpr int SB = 8;                    // values a thread stages per batch
constexpr int STAGE_BYTES = 64 * 1024;   // the staging budget
constexpr int PIX_MAX = 1 << 22;         // H, W: pixel centres x + 0.5 and the window bounds stay well inside fp32
constexpr int TV_BLOCKS = 1024;

struct BgArgs {
  const float* in;
  const float* grids;
  const float* g_out;
  float* out;
  float* g_in;
  float* g_grids;
  int64_t s[4];  // element strides of `in` (and g_in): view, channel, row, column
  int W, H, P, bpv, layout;
  int L, Gh, Gw;
  int ny_max;  // vertex rows the launch has LDS for; 0: no staging
};

struct Cell {
  int i0;
  float t;
};
// pixel i of n -> grid coordinate in [0, g - 1)
__device__ inline float coord(int i, int n, int g) { return ((float)i + 0.5f) / (float)n * (float)(g - 1); }
// f in [0, g - 1] -> its cell corner and fraction
__device__ inline Cell cell_of(float f, int g) {
  const int i0 = min((int)f, g - 2);
  return {i0, f - (float)i0};
}
__device__ inline float lw(int k) { return k == 0 ? 0.299f : (k == 1 ? 0.587f : 0.114f); }  // the luminance weights
__device__ inline float luminance(float r, float g, float b) { return fmaf(lw(2), b, fmaf(lw(1), g, lw(0) * r)); }
__device__ inline float level_of(float lum, int L) { return fminf(fmaxf(lum, 0.f), 1.f) * (float)(L - 1); }

// where a workgroup of the two streams finds its corner matrices
struct GridSrc {
  const float* g;  // the view's grid in global memory
  int64_t cs;      // its channel stride L Gh Gw
  int Gh, Gw, L, iy_lo;
  bool staged;
  __device__ inline void get(int x, int y, int z, float (&m)[12]) const {
    if (staged) {
      const float4* q = stage + (((y - iy_lo) * Gw + x) * L + z) * 3;
      const float4 q0 = q[0], q1 = q[1], q2 = q[2];
      m[0] = q0.x, m[1] = q0.y, m[2] = q0.z, m[3] = q0.w, m[4] = q1.x, m[5] = q1.y, m[6] = q1.z, m[7] = q1.w;
      m[8] = q2.x, m[9] = q2.y, m[10] = q2.z, m[11] = q2.w;
    } else {
      const float* p = g + ((int64_t)(z * Gh + y) * Gw + x);
#pragma unroll
      for (int ch = 0; ch < 12; ++ch) m[ch] = p[ch * cs];
    }
  }
};

// stage the vertex rows the pixels p0 .. p1 - 1 of view v can reach (every thread of the workgroup calls this)
__device__ inline GridSrc open_grid(const BgArgs& a, int v, int p0, int p1) {
  GridSrc src;
  src.cs = (int64_t)a.L * a.Gh * a.Gw;
  src.g = a.grids + (int64_t)v * 12 * src.cs;
  src.Gh = a.Gh, src.Gw = a.Gw, src.L = a.L;
  src.iy_lo = cell_of(coord(p0 / a.W, a.H, a.Gh), a.Gh).i0;
  const int ny = cell_of(coord((p1 - 1) / a.W, a.H, a.Gh), a.Gh).i0 + 2 - src.iy_lo;
  src.staged = ny <= a.ny_max;
  if (src.staged) {
    float* lds = reinterpret_cast<float*>(stage);
    const int n = ny * a.L * 12 * a.Gw;
    for (int e0 = threadIdx.x; e0 < n; e0 += NT * SB) {  // e = ((row, level), channel, column): columns are consecutive in memory
      float val[SB];
      int dst[SB];
#pragma unroll
      for (int j = 0; j < SB; ++j) {  // (the loads of a batch are issued together: one load per store would be a chain of memory latencies)
        const int e = e0 + j * NT;
        if (e < n) {
          const int q = e / a.Gw, x = e - q * a.Gw, ch = q % 12, q2 = q / 12, z = q2 % a.L, yl = q2 / a.L;
          dst[j] = ((yl * a.Gw + x) * a.L + z) * 12 + ch;
          val[j] = src.g[ch * src.cs + ((int64_t)(z * a.Gh + src.iy_lo + yl) * a.Gw + x)];
        }
      }
#pragma unroll
      for (int j = 0; j < SB; ++j) {
        if (e0 + j * NT < n) lds[dst[j]] = val[j];
      }
    }
    __syncthreads();
  }
  return src;
}

// M: the matrix of one pixel; D = dM/dz: the xy-interpolated level z0 + 1 minus the xy-interpolated level z0
__device__ inline void slice(const GridSrc& src, Cell cx, Cell cy, Cell cz, float (&M)[12], float (&D)[12]) {
  float A[2][12];
#pragma unroll
  for (int dz = 0; dz < 2; ++dz) {
    float r[2][12];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      float p[12], q[12];
      src.get(cx.i0, cy.i0 + dy, cz.i0 + dz, p);
      src.get(cx.i0 + 1, cy.i0 + dy, cz.i0 + dz, q);
#pragma unroll
      for (int ch = 0; ch < 12; ++ch) r[dy][ch] = fmaf(cx.t, q[ch] - p[ch], p[ch]);
    }
#pragma unroll
    for (int ch = 0; ch < 12; ++ch) A[dz][ch] = fmaf(cy.t, r[1][ch] - r[0][ch], r[0][ch]);
  }
#pragma unroll
  for (int ch = 0; ch < 12; ++ch) {
    D[ch] = A[1][ch] - A[0][ch];
    M[ch] = fmaf(cz.t, D[ch], A[0][ch]);
  }
}

// row c of a 3 x 4 matrix applied to (r, g, b, 1), in exposure_fwd_kernel's order
__device__ inline float affine(const float (&M)[12], int c, float r, float g, float b) {
  return fmaf(M[4 * c + 2], b, fmaf(M[4 * c + 1], g, fmaf(M[4 * c], r, M[4 * c + 3])));
}

// GIN false: the slice (out is written); true: the backward to the image (g_in is written)
template <bool GIN>
__global__ __launch_bounds__(NT) void bilagrid_stream_kernel(BgArgs a) {
  const int v = blockIdx.y, p0 = blockIdx.x * CHUNK;
  const GridSrc src = open_grid(a, v, p0, min(p0 + CHUNK, a.P));
  const float* in = a.in + v * a.s[0];
  float* g_in = GIN ? a.g_in + v * a.s[0] : nullptr;
  const float* g_out = GIN ? a.g_out + (int64_t)v * 3 * a.P : nullptr;
  float* out = GIN ? nullptr : a.out + (int64_t)v * 3 * a.P;
  const bool vin = strided_vec(in, a), vgin = GIN && strided_vec(g_in, a), vpl = planes_vec(GIN ? g_out : out, a.P);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i0 = p0 + r * NT * PX + threadIdx.x * PX;
    if (i0 >= a.P) break;
    float x[3][PX], g[3][PX], y[3][PX];
    load3(in, a, i0, vin, x);
    if (GIN) load_planes(g_out, a.P, i0, vpl, g);
    int py = i0 / a.W, px = i0 - py * a.W;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (i0 + k < a.P) {
        const float lum = luminance(x[0][k], x[1][k], x[2][k]);
        float M[12], D[12];
        slice(src, cell_of(coord(px, a.W, a.Gw), a.Gw), cell_of(coord(py, a.H, a.Gh), a.Gh), cell_of(level_of(lum, a.L), a.L), M, D);
        if (GIN) {
          float S = g[0][k] * affine(D, 0, x[0][k], x[1][k], x[2][k]);
          S = fmaf(g[1][k], affine(D, 1, x[0][k], x[1][k], x[2][k]), S);
          S = fmaf(g[2][k], affine(D, 2, x[0][k], x[1][k], x[2][k]), S);
          S = lum > 0.f && lum < 1.f ? S * (float)(a.L - 1) : 0.f;
#pragma unroll
          for (int j = 0; j < 3; ++j) y[j][k] = fmaf(lw(j), S, fmaf(M[8 + j], g[2][k], fmaf(M[4 + j], g[1][k], M[j] * g[0][k])));
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) y[c][k] = affine(M, c, x[0][k], x[1][k], x[2][k]);
        }
      } else {
        y[0][k] = y[1][k] = y[2][k] = 0.f;
      }
      if (++px == a.W) px = 0, ++py;
    }
    if (GIN)
      store3(g_in, a, i0, vgin, y);
    else
      store_planes(out, a.P, i0, vpl, y);
  }
}

// the weight of vertex i for a pixel in cell c
__device__ inline float vertex_weight(Cell c, int i) { return c.i0 == i ? 1.f - c.t : (c.i0 + 1 == i ? c.t : 0.f); }

// the pixels n * s - 0.5 of vertex coordinate n, clamped to the image, with a margin the membership test absorbs
__device__ inline void window(int i, int n_pix, int g, int& lo, int& hi) {
  const double s = (double)n_pix / (double)(g - 1);
  lo = max((int)floor((double)(i - 1) * s - 0.5) - 1, 0);
  hi = min((int)ceil((double)(i + 1) * s - 0.5) + 1, n_pix - 1);
}

__global__ __launch_bounds__(NT) void bilagrid_ggrid_kernel(BgArgs a) {
  __shared__ double red[12 * 4];
  const int v = blockIdx.y, iy = blockIdx.x / a.Gw, ix = blockIdx.x - iy * a.Gw;
  int ylo, yhi, xlo, xhi;
  window(iy, a.H, a.Gh, ylo, yhi);
  window(ix, a.W, a.Gw, xlo, xhi);
  const int ww = xhi - xlo + 1, n = (yhi - ylo + 1) * ww;  // (a clamped window holds at least one pixel, at most the image)
  const float* in = a.in + v * a.s[0];
  const float* g_out = a.g_out + (int64_t)v * 3 * a.P;
  const int64_t cs = (int64_t)a.L * a.Gh * a.Gw;
  float* dst = a.g_grids + (int64_t)v * 12 * cs + iy * a.Gw + ix;
  for (int lb = 0; lb < a.L; lb += LB) {
    float acc[LB][12];
#pragma unroll
    for (int j = 0; j < LB; ++j) {
#pragma unroll
      for (int ch = 0; ch < 12; ++ch) acc[j][ch] = 0.f;
    }
    for (int idx0 = threadIdx.x; idx0 < n; idx0 += NT * PF) {
      float wxy[PF], col[PF][3], g[PF][3];
#pragma unroll
      for (int u = 0; u < PF; ++u) {  // (PF pixels' loads are issued together; a thread still adds its pixels in index order)
        const int idx = idx0 + u * NT;
        wxy[u] = 0.f;
        if (idx < n) {
          const int yy = idx / ww, y = ylo + yy, x = xlo + idx - yy * ww;
          wxy[u] = vertex_weight(cell_of(coord(y, a.H, a.Gh), a.Gh), iy) * vertex_weight(cell_of(coord(x, a.W, a.Gw), a.Gw), ix);
          if (wxy[u] != 0.f) {  // (a pixel that is not this vertex's is not read)
            const float* p = in + y * a.s[2] + x * a.s[3];
            const int i = y * a.W + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) col[u][c] = p[c * a.s[1]], g[u][c] = g_out[c * (int64_t)a.P + i];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        if (wxy[u] != 0.f) {
          const float fz = level_of(luminance(col[u][0], col[u][1], col[u][2]), a.L);
#pragma unroll
          for (int j = 0; j < LB; ++j) {
            const float w = wxy[u] * fmaxf(0.f, 1.f - fabsf(fz - (float)(lb + j)));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float wg = w * g[u][c];
              acc[j][4 * c] = fmaf(wg, col[u][0], acc[j][4 * c]);
              acc[j][4 * c + 1] = fmaf(wg, col[u][1], acc[j][4 * c + 1]);
              acc[j][4 * c + 2] = fmaf(wg, col[u][2], acc[j][4 * c + 2]);
              acc[j][4 * c + 3] += wg;
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      double s[12];
#pragma unroll
      for (int ch = 0; ch < 12; ++ch) s[ch] = (double)acc[j][ch];
      block_reduce<Reduce::Sum>(s, red);
      if (threadIdx.x == 0 && lb + j < a.L) {
#pragma unroll
        for (int ch = 0; ch < 12; ++ch) dst[ch * cs + (int64_t)(lb + j) * a.Gh * a.Gw] = (float)s[ch];
      }
    }
  }
}

struct TvArgs {
  const float* A;
  float* g;
  double* partials;
  int64_t N;
  int L, Gh, Gw;
  double cz, cy, cx;  // 1 / (V x the element count of one view's differenced tensor), per axis
  double scale2;      // 2 scale
};

__global__ __launch_bounds__(NT) void bilagrid_tv_kernel(TvArgs a) {
  __shared__ double red[4];
  const int64_t sy = a.Gw, sz = (int64_t)a.Gh * a.Gw;
  double s[1] = {0.0};
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < a.N; e += (int64_t)gridDim.x * NT) {
    const int64_t q = e / a.Gw, q2 = q / a.Gh;
    const int x = (int)(e - q * a.Gw), y = (int)(q - q2 * a.Gh), z = (int)(q2 % a.L);
    const float c = a.A[e];
    double gr = 0.0;  // sum over the axes of c_axis ((c - previous) - (next - c))
    if (z + 1 < a.L) {
      const double d = (double)(a.A[e + sz] - c);
      s[0] += a.cz * (d * d), gr -= a.cz * d;
    }
    if (z > 0) gr += a.cz * (double)(c - a.A[e - sz]);
    if (y + 1 < a.Gh) {
      const double d = (double)(a.A[e + sy] - c);
      s[0] += a.cy * (d * d), gr -= a.cy * d;
    }
    if (y > 0) gr += a.cy * (double)(c - a.A[e - sy]);
    if (x + 1 < a.Gw) {
      const double d = (double)(a.A[e + 1] - c);
      s[0] += a.cx * (d * d), gr -= a.cx * d;
    }
    if (x > 0) gr += a.cx * (double)(c - a.A[e - 1]);
    if (a.g) a.g[e] = (float)((double)a.g[e] + a.scale2 * gr);
  }
  block_reduce<Reduce::Sum>(s, red);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(NT) void bilagrid_tv_sum_kernel(const double* partials, int n, float* value) {
  __shared__ double red[4];
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += NT) s[0] += partials[i];
  block_reduce<Reduce::Sum>(s, red);
  if (threadIdx.x == 0) value[0] = (float)s[0];
}

int tv_blocks(int64_t N) { return (int)((N + NT - 1) / NT < TV_BLOCKS ? (N + NT - 1) / NT : TV_BLOCKS); }

int grid_shape_ok(const char* who, int V, int L, int Gh, int Gw) {
  SIU3R_CHECK(V > 0 && V <= 65535, "%s: %d views (1 .. 65535)", who, V);
  SIU3R_CHECK(L >= 2 && L <= LMAX, "%s: %d levels (2 .. %d)", who, L, LMAX);
  SIU3R_CHECK(Gh >= 2 && Gh <= GMAX && Gw >= 2 && Gw <= GMAX, "%s: a %d x %d grid (2 .. %d per axis)", who, Gh, Gw, GMAX);
  return 0;
}

// what both slice entry points check and derive
int bilagrid_args(const char* who, const float* in, const int64_t* st, const float* grids, int V, int H, int W, int L, int Gh, int Gw, BgArgs& a) {
  SIU3R_CHECK(in && st && grids, "%s: null pointer", who);
  SIU3R_CHECK(H > 0 && W > 0, "%s: empty input [%d,3,%d,%d]", who, V, H, W);
  if (int rc = grid_shape_ok(who, V, L, Gh, Gw)) return rc;
  SIU3R_CHECK((int64_t)H * W <= 0x7fffffff - CHUNK, "%s: %d x %d pixels per view exceed 32-bit indexing", who, H, W);
  SIU3R_CHECK(H <= PIX_MAX && W <= PIX_MAX, "%s: %d x %d: an image axis above %d pixels has no exact fp32 pixel centres", who, H, W, PIX_MAX);
  for (int i = 0; i < 4; ++i) SIU3R_CHECK(st[i] >= 0, "%s: negative strides are not supported", who);
  memset(&a, 0, sizeof(a));
  a.in = in, a.grids = grids;
  for (int i = 0; i < 4; ++i) a.s[i] = st[i];
  a.W = W, a.H = H, a.P = H * W, a.L = L, a.Gh = Gh, a.Gw = Gw;
  a.bpv = (int)(((int64_t)H * W + CHUNK - 1) / CHUNK);
  const bool rows_dense = H == 1 || st[2] == (int64_t)W * st[3];
  a.layout = st[3] == 1 && rows_dense ? PLANES : (st[1] == 1 && st[3] == 3 && rows_dense ? PIXELS : STRIDED);
  const int rows = (CHUNK + W - 2) / W + 1 < H ? (CHUNK + W - 2) / W + 1 : H;  // image rows CHUNK consecutive pixels can touch
  const int64_t ny = (int64_t)((double)(rows - 1) * (Gh - 1) / H) + 4;
  a.ny_max = (int)(ny < Gh ? ny : Gh);
  if ((int64_t)a.ny_max * Gw * L * 48 > STAGE_BYTES) a.ny_max = 0;
  return 0;
}

}  // namespace

extern "C" int siu3r_bilagrid_apply(const float* in, const int64_t* in_strides, const float* grids, int V, int H, int W, int L, int Gh, int Gw,
                                    float* out, void* stream) {
  BgArgs a;
  if (int rc = bilagrid_args("bilagrid_apply", in, in_strides, grids, V, H, W, L, Gh, Gw, a)) return rc;
  SIU3R_CHECK(out, "bilagrid_apply: null pointer");
  a.out = out;
  hipLaunchKernelGGL((bilagrid_stream_kernel<false>), dim3((unsigned)a.bpv, (unsigned)V), dim3(NT), (size_t)a.ny_max * Gw * L * 48, (hipStream_t)stream, a);
  SIU3R_LAUNCH_CHECK("siu3r_bilagrid_apply");
  return 0;
}

extern "C" int siu3r_bilagrid_apply_bwd(const float* in, const int64_t* in_strides, const float* grids, const float* g_out, int V, int H, int W, int L,
                                        int Gh, int Gw, float* g_in, float* g_grids, void* stream) {
  BgArgs a;
  if (int rc = bilagrid_args("bilagrid_apply_bwd", in, in_strides, grids, V, H, W, L, Gh, Gw, a)) return rc;
  SIU3R_CHECK(g_out, "bilagrid_apply_bwd: null pointer");
  if (!g_in && !g_grids) return 0;
  a.g_out = g_out, a.g_in = g_in, a.g_grids = g_grids;
  hipStream_t s = (hipStream_t)stream;
  if (g_in) {
    hipLaunchKernelGGL((bilagrid_stream_kernel<true>), dim3((unsigned)a.bpv, (unsigned)V), dim3(NT), (size_t)a.ny_max * Gw * L * 48, s, a);
    SIU3R_LAUNCH_CHECK("siu3r_bilagrid_apply_bwd (image)");
  }
  if (g_grids) {
    hipLaunchKernelGGL(bilagrid_ggrid_kernel, dim3((unsigned)(Gh * Gw), (unsigned)V), dim3(NT), 0, s, a);
    SIU3R_LAUNCH_CHECK("siu3r_bilagrid_apply_bwd (grid)");
  }
  return 0;
}

extern "C" int64_t siu3r_bilagrid_tv_ws(int V, int L, int Gh, int Gw) {
  if (V <= 0 || V > 65535 || L < 2 || L > LMAX || Gh < 2 || Gh > GMAX || Gw < 2 || Gw > GMAX) return 0;
  return (int64_t)tv_blocks((int64_t)V * 12 * L * Gh * Gw) * (int64_t)sizeof(double);
}

extern "C" int siu3r_bilagrid_tv(const float* grids, int V, int L, int Gh, int Gw, float scale, float* g_grids, void* ws, float* value, void* stream) {
  SIU3R_CHECK(grids && value, "bilagrid_tv: null pointer");
  if (int rc = grid_shape_ok("bilagrid_tv", V, L, Gh, Gw)) return rc;
  SIU3R_CHECK(ws && ((uintptr_t)ws & 7) == 0, "bilagrid_tv: the workspace (siu3r_bilagrid_tv_ws bytes, 8-byte aligned) is missing");
  SIU3R_CHECK(scale == scale && scale - scale == 0.f, "bilagrid_tv: scale %g must be finite", (double)scale);
  TvArgs a;
  a.A = grids, a.g = g_grids, a.partials = (double*)ws, a.N = (int64_t)V * 12 * L * Gh * Gw, a.L = L, a.Gh = Gh, a.Gw = Gw;
  a.cz = 1.0 / ((double)V * 12 * (L - 1) * Gh * Gw), a.cy = 1.0 / ((double)V * 12 * L * (Gh - 1) * Gw), a.cx = 1.0 / ((double)V * 12 * L * Gh * (Gw - 1));
  a.scale2 = 2.0 * (double)scale;
  const int nb = tv_blocks(a.N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bilagrid_tv_kernel, dim3((unsigned)nb), dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_bilagrid_tv");
  hipLaunchKernelGGL(bilagrid_tv_sum_kernel, dim3(1), dim3(NT), 0, s, (const double*)a.partials, nb, value);
  SIU3R_LAUNCH_CHECK("siu3r_bilagrid_tv (final sum)");
  return 0;
}
