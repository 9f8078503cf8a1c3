// Per-Gaussian blend-contribution statistics for gfx950: the walk of composite_rgb_kernel (raster.hip) restated without colours.
//
// For every (view, Gaussian): the largest blending weight w = alpha * T the Gaussian reaches in any pixel of the view (wmax), the
// number of pixels that blend it (count) and the sum of its weights in fixed point, units of 2^-40 (wsum).  "Blends" is the forward's
// `reach && !sat`; a, nT and w are the forward's expressions in the forward's order (helpers from raster_shared.h), so every w is the
// very float the forward adds into its pixel.
//
// Everything is an integer reduction, hence bit-reproducible whatever the arrival order: w >= 0, so max(w) is the unsigned maximum of
// the bit patterns; w * 2^40 is exact in fp32 (a power-of-two scale) and its truncation to an integer is summed in 64 bits (2^23
// pixels x w < 1 stays below 2^63).  No float atomic anywhere.
//
// Reduction: three accumulators per staged entry live in LDS where the forward keeps the colour (8 bytes + 4 + 4 against 16).  The
// lanes that blend an entry go to its slot directly -- one LDS max and one 64-bit LDS add per lane, the count as one add per wave from
// a ballot, as the forward counts n_touched.  Same-address LDS atomics of a wave serialise over the lanes that issue them, and those
// are the pixels inside the alpha >= alpha_min footprint: a handful for the pixel-aligned Gaussians this project renders.  A wave
// reduction in front of the slot would pay its 2 x 6 cross-lane steps on every (wave, entry) for the sake of the few large splats; the
// kernel runs once per pruning event, not per iteration, so the short form was kept (DESIGN.md section 26 has the measured cost).
// After each walk the slots are flushed with one global integer atomic per (tile, Gaussian, non-zero statistic).
#include "common.h"
#include "raster_shared.h"

namespace {

typedef siu3r_raster_cam Cam;

// the staging constants of composite_rgb_kernel (the refill rounds of the two kernels are the same rounds)
constexpr int STG = 512;       // staging capacity (survivors awaiting the walk)
constexpr int STG_PULL = 192;  // refill while fewer than this are staged (<= STG - 256: one more slice always fits)
constexpr int FK = 4;          // slices of 256 entries tested per refill round

template <bool K3>
__global__ __launch_bounds__(256) void contrib_kernel(const Cam* __restrict__ cams, Geo geo, const int32_t* __restrict__ bin_start,
                                                      const uint2* __restrict__ entries, int64_t cap_e, const float* __restrict__ rec, int64_t G,
                                                      uint32_t* __restrict__ wmax, int32_t* __restrict__ count, unsigned long long* __restrict__ wsum) {
  // staged survivors: {mx, my, depth, id} {conic a, b, c, opacity} + quadrant mask, as in the forward; in place of the colour the three
  // accumulators of the entry
  __shared__ int s_m[STG];
  __shared__ __attribute__((aligned(16))) float s_a[STG][4];
  __shared__ __attribute__((aligned(16))) float s_co[STG][4];
  __shared__ unsigned long long s_sum[STG];
  __shared__ uint32_t s_max[STG];
  __shared__ int s_cnt[STG];
  __shared__ int s_wcnt[4][FK];
  __shared__ __attribute__((aligned(16))) unsigned short s_list[4][STG];
  const int v = blockIdx.y;
  const Cam& c = cams[v];
  const int tile = blockIdx.x, tx = tile % geo.gw, ty = tile / geo.gw;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t vg = (int64_t)v * G;
  // A view whose coarse-bin entries did not fit cap_e lost its farthest splats: no statistic of it can be trusted, so its wmax row is
  // POISONED (NaN) and count / wsum stay zero (nothing of the view is walked); the caller may read the overflow counters late
  if ((int64_t)bin_start[v * (geo.NB + 1) + geo.NB] > cap_e) {  // (uniform)
    for (int64_t g = (int64_t)tile * 256 + t; g < G; g += (int64_t)geo.T * 256) wmax[vg + g] = 0x7fc00000u;
    return;
  }
  const int bx = tx / geo.cb, by = ty / geo.cb, bin = by * geo.nbx + bx;
  const int rtx = tx - bx * geo.cb, rty = ty - by * geo.cb;
  const int lx = (lane & 7) + 8 * (wave & 1), ly = (lane >> 3) + 8 * (wave >> 1);  // wave = 8x8 quadrant
  const int px = tx * TILE + lx, py = ty * TILE + ly;
  const bool inside = px < c.width && py < c.height;
  const float pxf = (float)px + (K3 ? 0.5f : 0.0f), pyf = (float)py + (K3 ? 0.5f : 0.0f);
  const int64_t ebeg = bin_start[v * (geo.NB + 1) + bin];
  const int64_t eend = min((int64_t)bin_start[v * (geo.NB + 1) + bin + 1], cap_e);
  const uint2* ep = entries + (int64_t)v * cap_e;
  const float alpha_min = c.alpha_min, alpha_max = c.alpha_max, t_min = c.t_min;
  const float tile_x0 = (float)(tx * TILE), tile_y0 = (float)(ty * TILE);
  const int wbit = 1 << wave;
  float T = 1.0f;
  bool done = !inside;
  int staged = 0;
  int64_t base = ebeg;
  while (true) {
    if (__syncthreads_count(done) == 256) break;  // also fences the previous round's LDS reads (the flush included)
    // refill: the forward's, slice for slice (same survivors in the same slots of the same rounds)
    while (staged < STG_PULL && base < eend) {
      uint2 e[FK];
      bool pass[FK];
      unsigned long long m[FK];
#pragma unroll
      for (int k = 0; k < FK; ++k) {
        const int64_t i = base + k * 256 + t;
        e[k] = i < eend ? ep[i] : make_uint2(0, 0);
      }
#pragma unroll
      for (int k = 0; k < FK; ++k) {
        pass[k] = (base + k * 256 + t < eend) && entry_covers(e[k].y, rtx, rty);
        m[k] = __ballot(pass[k]);
        if (lane == 0) s_wcnt[wave][k] = __popcll(m[k]);
      }
      __syncthreads();
      int kk = 0, off_k[FK], run = staged;
#pragma unroll
      for (int k = 0; k < FK; ++k) {
        const int tk = s_wcnt[0][k] + s_wcnt[1][k] + s_wcnt[2][k] + s_wcnt[3][k];
        int o = run;
        for (int w = 0; w < wave; ++w) o += s_wcnt[w][k];
        off_k[k] = o + __popcll(m[k] & ((1ull << lane) - 1ull));
        if (kk == k && run + tk <= STG) {  // slice k fits (slice 0 always does: staged < STG_PULL <= STG - 256)
          kk = k + 1;
          run += tk;
        }
      }
#pragma unroll
      for (int k = 0; k < FK; ++k) {
        if (k < kk && pass[k]) {
          const int off = off_k[k];
          const float4* rp = (const float4*)(rec + 12 * (vg + e[k].x));
          float4 r0 = rp[0];
          const float4 r1 = rp[1];
          r0.w = __int_as_float((int)e[k].x);
          *(float4*)s_a[off] = r0;
          *(float4*)s_co[off] = r1;
          s_sum[off] = 0ull;
          s_max[off] = 0u;
          s_cnt[off] = 0;
          s_m[off] = quadrant_mask<K3>(r0, r1, alpha_min, tile_x0, tile_y0);
        }
      }
      staged = run;
      base += 256 * kk;
      __syncthreads();
    }
    if (staged == 0) break;
    // this wave's own list (order kept) of the staged survivors that can reach its quadrant (wave-local, as in the forward)
    int nq = 0;
    for (int b = 0; b < staged; b += 64) {
      const int i = b + lane;
      const bool hit = i < staged && (s_m[i] & wbit);
      const unsigned long long mh = __ballot(hit);
      if (hit) s_list[wave][nq + __popcll(mh & ((1ull << lane) - 1ull))] = (unsigned short)i;
      nq += __popcll(mh);
    }
    __builtin_amdgcn_wave_barrier();
    // The walk: one entry per iteration (the forward's four-entry software pipeline buys nothing the statistics could use: the per-lane
    // operations and their order are what has to agree, and they do)
    const unsigned short* lst = s_list[wave];
    for (int i = 0; i < nq; ++i) {
      const int j = lst[i];
      const float4 A = *(const float4*)s_a[j], Q = *(const float4*)s_co[j];
      const float dx = A.x - pxf, dy = A.y - pyf;
      const float power = -conic_sigma(Q.x, Q.y, Q.z, dx, dy);
      const float a = fminf(alpha_max, Q.w * exp_det_sel(power));
      const float nT = __builtin_fmaf(-T, a, T);  // T (1 - a)
      const bool reach = !done && !(power > 0.0f) && !(a < alpha_min);
      const bool sat = reach && (K3 ? (nT <= t_min) : (nT < t_min));
      done = done || sat;
      if (reach && !sat) {
        const float w = a * T;
        atomicMax(&s_max[j], __float_as_uint(w));
        if (wsum) atomicAdd(&s_sum[j], (unsigned long long)(w * 0x1p40f));
        if (count) {
          const unsigned long long mc = __ballot(true);  // the lanes that reached this point
          if (lane == (int)__ffsll((long long)mc) - 1) atomicAdd(&s_cnt[j], (int)__popcll(mc));
        }
        T = nT;
      }
      if (__ballot(!done) == 0ull) break;
    }
    __syncthreads();
    for (int j = t; j < staged; j += 256) {
      const int64_t o = vg + __float_as_int(s_a[j][3]);
      const uint32_t mx = s_max[j];
      if (mx) atomicMax(&wmax[o], mx);
      if (count) {
        const int n = s_cnt[j];
        if (n) atomicAdd(&count[o], n);
      }
      if (wsum) {
        const unsigned long long q = s_sum[j];
        if (q) atomicAdd(&wsum[o], q);
      }
    }
    staged = 0;
  }
}

// every view of a call: one camera family, one frame size
inline int check_views(const siu3r_raster_cam* cams, int V, const char* who) {
  SIU3R_CHECK(cams && V >= 1 && V <= 65535, "%s: bad view array (V = %d)", who, V);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK((cams[v].mode == 0 || cams[v].mode == 1) && cams[v].mode == cams[0].mode && cams[v].width == cams[0].width &&
                    cams[v].height == cams[0].height && cams[v].width > 0 && cams[v].height > 0,
                "%s: the statistics cover one family (view 0: mode %d) with one frame size per call (view %d: mode %d)", who, cams[0].mode, v, cams[v].mode);
  return 0;
}

}  // namespace

extern "C" int siu3r_raster_contrib(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                    const void* entries, int64_t cap_e, const float* rec, float* wmax, int32_t* count, uint64_t* wsum, void* stream) {
  if (int rc = check_views(cams_host, V, "raster_contrib")) return rc;
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "raster_contrib: G = %ld out of range", (long)G);
  if (G == 0) return 0;
  SIU3R_CHECK(cams_dev && bin_start && entries && rec && wmax, "raster_contrib: null pointer");
  SIU3R_CHECK(cap_e > 0, "raster_contrib: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)V * (size_t)G;
  if (hipMemsetAsync(wmax, 0, sizeof(float) * n, s) != hipSuccess || (count && hipMemsetAsync(count, 0, sizeof(int32_t) * n, s) != hipSuccess) ||
      (wsum && hipMemsetAsync(wsum, 0, sizeof(uint64_t) * n, s) != hipSuccess)) {
    siu3r_set_error("raster_contrib: memset failed");
    return 2;
  }
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  if (cams_host[0].mode == 1)
    hipLaunchKernelGGL(contrib_kernel<true>, dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, bin_start, (const uint2*)entries, cap_e, rec, G,
                       (uint32_t*)wmax, count, (unsigned long long*)wsum);
  else
    hipLaunchKernelGGL(contrib_kernel<false>, dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, bin_start, (const uint2*)entries, cap_e, rec, G,
                       (uint32_t*)wmax, count, (unsigned long long*)wsum);
  SIU3R_LAUNCH_CHECK("siu3r_raster_contrib");
  return 0;
}
