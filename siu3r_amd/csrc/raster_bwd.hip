// Backward pass of the K2 splat rasterizer (diff-gaussian-rasterization conventions, mode 0): the gradients of colour-with-background,
// depth (sum of w z) and accumulated opacity with respect to the per-(view, Gaussian) screen-space record, and from there to the
// Gaussians (means, covariances, opacities, SH coefficients or precomputed colours) and to a left se(3) perturbation of every view's
// world->camera pose.
//
//   composite bwd   one 16x16 workgroup per (tile, view), like composite_rgb_kernel.  It re-walks the tile's coarse-bin entries front to
//                   back in the forward's order, with the forward's quadrant masks and the same alpha / transmittance operations
//                   (raster_shared.h), so every pixel stops at the same entry as the forward did.  The part of each output that lies
//                   BEHIND an entry (suffix) is the forward's saved total minus the running prefix.  Per entry, each wave sums its 64
//                   pixels' ten gradient terms by cross-lane reduction (skipping terms that are zero on the whole wave) and adds them into
//                   an LDS slot of the staged entry; after the slice the workgroup adds every non-zero slot to global memory: one float atomic per
//                   (tile, Gaussian, term).
//   projection bwd  one thread per Gaussian, looping over the call's views like project_kernel: per-Gaussian gradients are plain stores.
//                   The six pose terms of a view are summed per workgroup into a partial row; pose_reduce_kernel sums the rows.
// The gradient is that of the function the forward computes, on the branch it took: culling, tile rects, the alpha_min cut-off,
// saturation and the alpha_max clamp are held constant (no gradient through a clamped alpha); the limx / limy clamp of the Jacobian
// passes no gradient to the clamped component; a colour clamped at 0 passes none to its SH coefficients.
#include "common.h"
#include "raster_shared.h"
#include "raster_bwd_shared.h"

namespace {

typedef siu3r_raster_cam Cam;

// ---- composite backward ------------------------------------------------------------------------------------------------------------
constexpr int BSTG = 256;  // entries staged per slice
// K3 (compile time): the gsplat family's conventions on the same walk, as composite_rgb_kernel<NT, K3> -- pixel centres at +0.5, saturation
// test nT <= t_min, channel-last [V,H,W,3] colours and their gradient, no depth (depth / g_depth unused), no background (blended outside).
template <bool K3 = false>
__global__ __launch_bounds__(256) void composite_rgb_bwd_kernel(const Cam* __restrict__ cams, Geo geo, const int32_t* __restrict__ bin_start,
                                                                const uint2* __restrict__ entries, int64_t cap_e, const float* __restrict__ rec, int64_t G,
                                                                const float* __restrict__ image, const float* __restrict__ depth,
                                                                const float* __restrict__ alpha, const float* __restrict__ g_image,
                                                                const float* __restrict__ g_depth, const float* __restrict__ g_alpha,
                                                                float* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) float s_a[BSTG][4];   // mx, my, depth, id
  __shared__ __attribute__((aligned(16))) float s_co[BSTG][4];  // conic a, b, c, opacity
  __shared__ __attribute__((aligned(16))) float s_c[BSTG][4];   // r, g, b
  __shared__ int s_m[BSTG];                                     // quadrant mask (the forward's)
  __shared__ float s_g[BSTG][GR_N];                             // the tile's summed gradient terms per staged entry
  __shared__ int s_wcnt[4];
  const int v = blockIdx.y;
  const Cam& c = cams[v];
  const int tile = blockIdx.x, tx = tile % geo.gw, ty = tile / geo.gw;
  const int bx = tx / geo.cb, by = ty / geo.cb, bin = by * geo.nbx + bx;
  const int rtx = tx - bx * geo.cb, rty = ty - by * geo.cb;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lx = (lane & 7) + 8 * (wave & 1), ly = (lane >> 3) + 8 * (wave >> 1);
  const int px = tx * TILE + lx, py = ty * TILE + ly;
  const bool inside = px < c.width && py < c.height;
  const float pxf = (float)px + (K3 ? 0.5f : 0.0f), pyf = (float)py + (K3 ? 0.5f : 0.0f);
  const int64_t ebeg = bin_start[v * (geo.NB + 1) + bin];
  const int64_t eend = min((int64_t)bin_start[v * (geo.NB + 1) + bin + 1], cap_e);
  const uint2* ep = entries + (int64_t)v * cap_e;
  const int64_t vg = (int64_t)v * G;
  const float alpha_min = c.alpha_min, alpha_max = c.alpha_max, t_min = c.t_min;
  const float tile_x0 = (float)(tx * TILE), tile_y0 = (float)(ty * TILE);
  const int wbit = 1 << wave;
  // upstream gradients and the forward's totals of this pixel
  float gC0 = 0.f, gC1 = 0.f, gC2 = 0.f, gD = 0.f, gO = 0.f, tC0 = 0.f, tC1 = 0.f, tC2 = 0.f, tD = 0.f, tO = 0.f;
  if (inside && K3) {
    const size_t hw = (size_t)c.width * c.height, pix = (size_t)py * c.width + px;
    const size_t o = ((size_t)v * hw + pix) * 3;
    gC0 = g_image[o];
    gC1 = g_image[o + 1];
    gC2 = g_image[o + 2];
    gO = g_alpha[(size_t)v * hw + pix];
    tC0 = image[o];
    tC1 = image[o + 1];
    tC2 = image[o + 2];
    tO = alpha[(size_t)v * hw + pix];
  } else if (inside) {
    const size_t hw = (size_t)c.width * c.height, pix = (size_t)py * c.width + px;
    gC0 = g_image[(size_t)v * 3 * hw + pix];
    gC1 = g_image[(size_t)v * 3 * hw + hw + pix];
    gC2 = g_image[(size_t)v * 3 * hw + 2 * hw + pix];
    gD = g_depth[(size_t)v * hw + pix];
    gO = g_alpha[(size_t)v * hw + pix];
    tC0 = image[(size_t)v * 3 * hw + pix];
    tC1 = image[(size_t)v * 3 * hw + hw + pix];
    tC2 = image[(size_t)v * 3 * hw + 2 * hw + pix];
    tD = depth[(size_t)v * hw + pix];
    tO = alpha[(size_t)v * hw + pix];
  }
  float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, O = 0.f;
  // a pixel with no upstream gradient contributes nothing: it leaves the walk at once (other pixels' chains do not depend on it)
  bool done = !inside || (gC0 == 0.f && gC1 == 0.f && gC2 == 0.f && gD == 0.f && gO == 0.f);
  int64_t base = ebeg;
  while (true) {
    if (__syncthreads_count(done) == 256 || base >= eend) break;  // (uniform; also fences the previous slice's LDS reads)
    // stage the slice's entries that cover this tile, order kept (ballot + prefix popcount)
    const int64_t i = base + t;
    const uint2 e = i < eend ? ep[i] : make_uint2(0, 0);
    const bool pass = i < eend && entry_covers(e.y, rtx, rty);
    const unsigned long long m = __ballot(pass);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += s_wcnt[w];
      n += s_wcnt[w];
    }
    if (pass) {
      const float4* rp = (const float4*)(rec + 12 * (vg + e.x));
      float4 r0 = rp[0];
      const float4 r1 = rp[1];
      const float4 r2 = rp[2];
      r0.w = __int_as_float((int)e.x);
      *(float4*)s_a[off] = r0;
      *(float4*)s_co[off] = r1;
      *(float4*)s_c[off] = r2;
      // the forward's footprint box, the same expression (composite_rgb_kernel): a wave skips exactly the entries the forward's wave skipped
      int mk = 15;
      const float L = __logf(r1.w / alpha_min);
      const float det = conic_det(r1.x, r1.y, r1.z);
      if (L <= 0.f) {
        mk = 0;
      } else if (det > 0.f) {
        const float ex = sqrtf(2.f * L * r1.z / det) * 1.01f + (K3 ? 0.55f : 0.05f), ey = sqrtf(2.f * L * r1.x / det) * 1.01f + (K3 ? 0.55f : 0.05f);
        const float x0 = r0.x - ex - tile_x0, x1 = r0.x + ex - tile_x0, y0 = r0.y - ey - tile_y0, y1 = r0.y + ey - tile_y0;
        const int cx = (x0 <= 7.f && x1 >= 0.f ? 1 : 0) | (x0 <= 15.f && x1 >= 8.f ? 2 : 0);
        const int cy = (y0 <= 7.f && y1 >= 0.f ? 1 : 0) | (y0 <= 15.f && y1 >= 8.f ? 2 : 0);
        mk = ((cy & 1) ? cx : 0) | ((cy & 2) ? (cx << 2) : 0);
      }
      s_m[off] = mk;
#pragma unroll
      for (int k = 0; k < GR_N; ++k) s_g[off][k] = 0.f;
    }
    base += 256;
    __syncthreads();
    if (__ballot(!done) != 0ull) {
      for (int j = 0; j < n; ++j) {
        if (!(s_m[j] & wbit)) continue;  // (uniform per wave)
        const float4 A = *(const float4*)s_a[j], Q = *(const float4*)s_co[j];
        const float dx = A.x - pxf, dy = A.y - pyf;
        const float power = -conic_sigma(Q.x, Q.y, Q.z, dx, dy);
        const float ex = exp_det_sel(power);
        const float a = fminf(alpha_max, Q.w * ex);
        const float nT = __builtin_fmaf(-T, a, T);
        const bool reach = !done && !(power > 0.0f) && !(a < alpha_min);
        const bool sat = reach && (K3 ? (nT <= t_min) : (nT < t_min));
        done = done || sat;
        const bool blend = reach && !sat;
        float gv[GR_N];
#pragma unroll
        for (int k = 0; k < GR_N; ++k) gv[k] = 0.f;
        if (blend) {
          const float w = a * T;
          const float4 Cj = *(const float4*)s_c[j];
          C0 = __builtin_fmaf(Cj.x, w, C0);
          C1 = __builtin_fmaf(Cj.y, w, C1);
          C2 = __builtin_fmaf(Cj.z, w, C2);
          D = __builtin_fmaf(A.z, w, D);
          O += w;
          // d loss / d alpha = T (g . c_j) - (g . everything behind j) / (1 - alpha)
          const float behind = gC0 * (tC0 - C0) + gC1 * (tC1 - C1) + gC2 * (tC2 - C2) + gD * (tD - D) + gO * (tO - O);
          const float dLda = T * (gC0 * Cj.x + gC1 * Cj.y + gC2 * Cj.z + gD * A.z + gO) - behind / (1.0f - a);
          gv[GR_R] = gC0 * w;
          gv[GR_G] = gC1 * w;
          gv[GR_B] = gC2 * w;
          gv[GR_Z] = gD * w;
          if (!(Q.w * ex > alpha_max)) {  // alpha clamped at alpha_max: constant
            gv[GR_OP] = dLda * ex;
            const float dLdp = dLda * a;  // d loss / d power
            gv[GR_CA] = -0.5f * dx * dx * dLdp;
            gv[GR_CC] = -0.5f * dy * dy * dLdp;
            gv[GR_CB] = -dx * dy * dLdp;
            gv[GR_MX] = -dLdp * (Q.x * dx + Q.y * dy);
            gv[GR_MY] = -dLdp * (Q.z * dy + Q.y * dx);
          }
          T = nT;
        }
        if (__ballot(blend) != 0ull) {
#pragma unroll
          for (int k = 0; k < GR_N; ++k) {
            // a term that is zero on the whole wave (no upstream gradient of that output here, alpha clamped) skips its sum
            if (__ballot(gv[k] != 0.f) == 0ull) continue;
            const float s = wave_sum(gv[k]);
            if (lane == 0 && s != 0.f) atomicAdd(&s_g[j][k], s);  // (up to four waves per slot)
          }
        }
        if (__ballot(!done) == 0ull) break;
      }
    }
    __syncthreads();
    // one global add per (tile, Gaussian, non-zero term): ten consecutive lanes cover one Gaussian's 40-byte row
    for (int q = t; q < n * GR_N; q += 256) {
      const int j = q / GR_N, k = q - j * GR_N;
      const float s = s_g[j][k];
      if (s != 0.f) atomicAdd(&grad[(vg + __float_as_int(s_a[j][3])) * GR_N + k], s);
    }
  }
}

// ---- projection backward -----------------------------------------------------------------------------------------------------------
// grad [V, G, GR_N] (composite backward) -> g_means [G,3], g_cov [G, cov_stride], g_opac [G], g_colors (the layout of colors),
// g_mean2d [V, G, 2] (optional: the pixel-space mean gradient), pose_part [gridDim.x, V, 6] (optional: per-workgroup sums of
// d loss / d (rho, theta) of a left perturbation w2c <- exp(xi^) w2c).
__global__ __launch_bounds__(256) void project_bwd_kernel(const Cam* __restrict__ cams, int V, int64_t G, const float* __restrict__ means,
                                                          const float* __restrict__ cov, int cov_stride, const float* __restrict__ opac,
                                                          const float* __restrict__ colors, int channels, int sh_planar,
                                                          const int32_t* __restrict__ rect, const float* __restrict__ grad, float* __restrict__ g_means,
                                                          float* __restrict__ g_cov, float* __restrict__ g_opac, float* __restrict__ g_colors,
                                                          float* __restrict__ g_mean2d, float* __restrict__ pose_part) {
  __shared__ float s_pose[4][6];
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = g < G;
  float m[3] = {0.f, 0.f, 0.f}, S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool tri = cov_stride == 6;
  if (live) {
    m[0] = means[3 * g];
    m[1] = means[3 * g + 1];
    m[2] = means[3 * g + 2];
    const float* cg = cov + (size_t)g * cov_stride;
    S[0] = cg[0]; S[1] = cg[1]; S[2] = cg[2]; S[3] = cg[tri ? 3 : 4]; S[4] = cg[tri ? 4 : 5]; S[5] = cg[tri ? 5 : 8];
  }
  const float* shp = colors + (size_t)(live ? g : 0) * channels * 3;
  auto coef = [&](int k, int ch) { return sh_planar ? shp[ch * 25 + k] : shp[k * 3 + ch]; };
  float gm[3] = {0.f, 0.f, 0.f}, gS[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gop = 0.f, gsh[75];
#pragma unroll
  for (int k = 0; k < 75; ++k) gsh[k] = 0.f;
  for (int v = 0; v < V; ++v) {
    const Cam& c = cams[v];
    float dpose[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t o = (int64_t)v * G + g;
    const int4 r = live ? *(const int4*)(rect + 4 * o) : make_int4(0, 0, 0, 0);
    if (live && (r.z - r.x) * (r.w - r.y) != 0) {
      float gr[GR_N];
#pragma unroll
      for (int k = 0; k < GR_N; ++k) gr[k] = grad[o * GR_N + k];
      if (g_mean2d) {
        g_mean2d[2 * o] = gr[GR_MX];
        g_mean2d[2 * o + 1] = gr[GR_MY];
      }
      const float* W = c.w2c;
      const float tx = W[0] * m[0] + W[1] * m[1] + W[2] * m[2] + W[3];
      const float ty = W[4] * m[0] + W[5] * m[1] + W[6] * m[2] + W[7];
      const float tz = W[8] * m[0] + W[9] * m[1] + W[10] * m[2] + W[11];
      const float fx = c.width / (2.0f * c.tanfovx), fy = c.height / (2.0f * c.tanfovy);
      const float limx = 1.3f * c.tanfovx, limy = 1.3f * c.tanfovy;
      const float rz = 1.0f / tz;
      const float txz = tx * rz, tyz = ty * rz;
      const float cxz = fminf(limx, fmaxf(-limx, txz)), cyz = fminf(limy, fmaxf(-limy, tyz));
      const float ctx = cxz * tz, cty = cyz * tz;
      const float j00 = fx * rz, j02 = -(fx * ctx) * rz * rz, j11 = fy * rz, j12 = -(fy * cty) * rz * rz;
      const float t0[3] = {j00 * W[0] + j02 * W[8], j00 * W[1] + j02 * W[9], j00 * W[2] + j02 * W[10]};
      const float t1[3] = {j11 * W[4] + j12 * W[8], j11 * W[5] + j12 * W[9], j11 * W[6] + j12 * W[10]};
      // Sigma t0, Sigma t1 (Sigma symmetric from the six entries)
      const float a[3] = {t0[0] * S[0] + t0[1] * S[1] + t0[2] * S[2], t0[0] * S[1] + t0[1] * S[3] + t0[2] * S[4], t0[0] * S[2] + t0[1] * S[4] + t0[2] * S[5]};
      const float b[3] = {t1[0] * S[0] + t1[1] * S[1] + t1[2] * S[2], t1[0] * S[1] + t1[1] * S[3] + t1[2] * S[4], t1[0] * S[2] + t1[1] * S[4] + t1[2] * S[5]};
      const float c00 = a[0] * t0[0] + a[1] * t0[1] + a[2] * t0[2] + c.dilation;
      const float c01 = a[0] * t1[0] + a[1] * t1[1] + a[2] * t1[2];
      const float c11 = b[0] * t1[0] + b[1] * t1[1] + b[2] * t1[2] + c.dilation;
      const float det = c00 * c11 - c01 * c01, rdet = 1.0f / det;
      const float ca = c11 * rdet, cb = -c01 * rdet, cc = c00 * rdet;
      // conic inverse
      const float dLddet = -(gr[GR_CA] * ca + gr[GR_CB] * cb + gr[GR_CC] * cc) * rdet;
      const float d00 = gr[GR_CC] * rdet + dLddet * c11, d11 = gr[GR_CA] * rdet + dLddet * c00, d01 = -gr[GR_CB] * rdet - 2.0f * dLddet * c01;
      // 2-D covariance = T Sigma T^T, T = J W (rows t0, t1)
      float dt0[3], dt1[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        dt0[i] = 2.0f * d00 * a[i] + d01 * b[i];
        dt1[i] = 2.0f * d11 * b[i] + d01 * a[i];
      }
      gS[0] += d00 * t0[0] * t0[0] + d01 * t0[0] * t1[0] + d11 * t1[0] * t1[0];
      gS[3] += d00 * t0[1] * t0[1] + d01 * t0[1] * t1[1] + d11 * t1[1] * t1[1];
      gS[5] += d00 * t0[2] * t0[2] + d01 * t0[2] * t1[2] + d11 * t1[2] * t1[2];
      gS[1] += 2.0f * d00 * t0[0] * t0[1] + d01 * (t0[0] * t1[1] + t0[1] * t1[0]) + 2.0f * d11 * t1[0] * t1[1];
      gS[2] += 2.0f * d00 * t0[0] * t0[2] + d01 * (t0[0] * t1[2] + t0[2] * t1[0]) + 2.0f * d11 * t1[0] * t1[2];
      gS[4] += 2.0f * d00 * t0[1] * t0[2] + d01 * (t0[1] * t1[2] + t0[2] * t1[1]) + 2.0f * d11 * t1[1] * t1[2];
      const float W0[3] = {W[0], W[1], W[2]}, W1[3] = {W[4], W[5], W[6]}, W2[3] = {W[8], W[9], W[10]};
      const float dj00 = dt0[0] * W0[0] + dt0[1] * W0[1] + dt0[2] * W0[2], dj02 = dt0[0] * W2[0] + dt0[1] * W2[1] + dt0[2] * W2[2];
      const float dj11 = dt1[0] * W1[0] + dt1[1] * W1[1] + dt1[2] * W1[2], dj12 = dt1[0] * W2[0] + dt1[1] * W2[1] + dt1[2] * W2[2];
      // d loss / d W through the covariance only (rows), for the rotation part of the pose gradient
      float GW[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        GW[0][i] = j00 * dt0[i];
        GW[1][i] = j11 * dt1[i];
        GW[2][i] = j02 * dt0[i] + j12 * dt1[i];
      }
      // Jacobian -> camera-space point (the clamp of txz / tyz passes nothing to the clamped component)
      float drz = dj00 * fx + dj11 * fy - 2.0f * fx * ctx * rz * dj02 - 2.0f * fy * cty * rz * dj12;
      const float dctx = -fx * rz * rz * dj02, dcty = -fy * rz * rz * dj12;
      float dtz = dctx * cxz + dcty * cyz + gr[GR_Z];
      const float dtxz = (cxz == txz) ? dctx * tz : 0.f, dtyz = (cyz == tyz) ? dcty * tz : 0.f;
      const float dtx = dtxz * rz, dty = dtyz * rz;
      drz += dtxz * tx + dtyz * ty;
      dtz += -drz * rz * rz;
      // mean2d through the full projection P (world space)
      const float* P = c.proj;
      const float hx = P[0] * m[0] + P[1] * m[1] + P[2] * m[2] + P[3];
      const float hy = P[4] * m[0] + P[5] * m[1] + P[6] * m[2] + P[7];
      const float hw = P[12] * m[0] + P[13] * m[1] + P[14] * m[2] + P[15];
      const float pw = 1.0f / (hw + 0.0000001f);
      const float sx = 0.5f * c.width * gr[GR_MX], sy = 0.5f * c.height * gr[GR_MY];
      const float dhx = sx * pw, dhy = sy * pw, dhw = -(sx * hx + sy * hy) * pw * pw;
      float gmp[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) gmp[i] = dhx * P[i] + dhy * P[4 + i] + dhw * P[12 + i];
      const float dp[3] = {dtx, dty, dtz};
#pragma unroll
      for (int i = 0; i < 3; ++i) gm[i] += W0[i] * dp[0] + W1[i] * dp[1] + W2[i] * dp[2] + gmp[i];
      gop += gr[GR_OP];
      if (pose_part) {
        // camera-space point gradient of the whole view: dp + W^-T gmp (P = proj w2c: the matching P moves with the pose);
        // W^-T = cofactor(W) / det(W), cofactor rows = cross products of W's rows
        float C0[3], C1[3], C2[3];
        cross3(W1, W2, C0);
        cross3(W2, W0, C1);
        cross3(W0, W1, C2);
        const float rdw = 1.0f / (W0[0] * C0[0] + W0[1] * C0[1] + W0[2] * C0[2]);
        const float gp[3] = {dp[0] + (C0[0] * gmp[0] + C0[1] * gmp[1] + C0[2] * gmp[2]) * rdw,
                             dp[1] + (C1[0] * gmp[0] + C1[1] * gmp[1] + C1[2] * gmp[2]) * rdw,
                             dp[2] + (C2[0] * gmp[0] + C2[1] * gmp[1] + C2[2] * gmp[2]) * rdw};
        const float pc[3] = {tx, ty, tz};
        float th[3];
        cross3(pc, gp, th);  // point part: d/dtheta of g . (theta x p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // covariance part: sum over W's columns of W_:k x GW_:k
          const float wc[3] = {W0[k], W1[k], W2[k]}, gc[3] = {GW[0][k], GW[1][k], GW[2][k]};
          float cr[3];
          cross3(wc, gc, cr);
          th[0] += cr[0];
          th[1] += cr[1];
          th[2] += cr[2];
        }
        dpose[0] = gp[0], dpose[1] = gp[1], dpose[2] = gp[2], dpose[3] = th[0], dpose[4] = th[1], dpose[5] = th[2];
      }
      // colour
      const float gcol[3] = {gr[GR_R], gr[GR_G], gr[GR_B]};
      if (c.sh_degree < 0) {
        gsh[0] += gcol[0];
        gsh[1] += gcol[1];
        gsh[2] += gcol[2];
      } else {
        const float ddx = m[0] - c.campos[0], ddy = m[1] - c.campos[1], ddz = m[2] - c.campos[2];
        const float len = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz), inv = 1.0f / len;
        const float x = ddx * inv, y = ddy * inv, z = ddz * inv;
        const int deg = c.sh_degree;
        const bool band4 = c.sh_band4 != 0;
        // which channels the +0.5 / clamp-at-0 left alive
        float rsum[3] = {0.5f, 0.5f, 0.5f};
        sh_basis(x, y, z, deg, band4, [&](int k, Dual bk) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) rsum[ch] += bk.v * coef(k, ch);
        });
        float gl[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gl[ch] = rsum[ch] < 0.0f ? 0.0f : gcol[ch];
        float gd[3] = {0.f, 0.f, 0.f};
        sh_basis(x, y, z, deg, band4, [&](int k, Dual bk) {
          float s = 0.f;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            gsh[3 * k + ch] += bk.v * gl[ch];
            s += gl[ch] * coef(k, ch);
          }
          gd[0] += s * bk.x;
          gd[1] += s * bk.y;
          gd[2] += s * bk.z;
        });
        // unit direction (m - campos) / |m - campos|
        const float dd = gd[0] * x + gd[1] * y + gd[2] * z;
        gm[0] += (gd[0] - x * dd) * inv;
        gm[1] += (gd[1] - y * dd) * inv;
        gm[2] += (gd[2] - z * dd) * inv;
      }
    }
    if (pose_part) {  // (uniform: every thread of the workgroup runs every view)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const float s = wave_sum(dpose[k]);
        if (lane == 0) s_pose[wave][k] = s;
      }
      __syncthreads();
      if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        pose_part[((int64_t)blockIdx.x * V + v) * 6 + k] = s_pose[0][k] + s_pose[1][k] + s_pose[2][k] + s_pose[3][k];
      }
      __syncthreads();
    }
  }
  if (!live) return;
  g_means[3 * g] = gm[0];
  g_means[3 * g + 1] = gm[1];
  g_means[3 * g + 2] = gm[2];
  float* gc = g_cov + (size_t)g * cov_stride;
  if (tri) {
#pragma unroll
    for (int k = 0; k < 6; ++k) gc[k] = gS[k];
  } else {  // [3,3]: the entries the forward reads (0, 1, 2, 4, 5, 8); the lower triangle is not read and gets no gradient
    gc[0] = gS[0]; gc[1] = gS[1]; gc[2] = gS[2]; gc[3] = 0.f; gc[4] = gS[3]; gc[5] = gS[4]; gc[6] = 0.f; gc[7] = 0.f; gc[8] = gS[5];
  }
  g_opac[g] = gop;
  float* gcp = g_colors + (size_t)g * channels * 3;
  if (sh_planar) {
#pragma unroll
    for (int k = 0; k < 25; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gcp[ch * 25 + k] = gsh[3 * k + ch];
  } else {
#pragma unroll
    for (int q = 0; q < 75; ++q)  // (channels <= 25: checked by the launcher)
      if (q < channels * 3) gcp[q] = gsh[q];
  }
}

// pose_part [nblk, V, 6] -> g_pose [V, 6]: one workgroup per view
__global__ __launch_bounds__(256) void pose_reduce_kernel(int V, int64_t nblk, const float* __restrict__ pose_part, float* __restrict__ g_pose) {
  __shared__ float s[4][6];
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += pose_part[(b * V + v) * 6 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float t = wave_sum(acc[k]);
    if (lane == 0) s[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 6) g_pose[v * 6 + threadIdx.x] = s[0][threadIdx.x] + s[1][threadIdx.x] + s[2][threadIdx.x] + s[3][threadIdx.x];
}

int check_k2_views(const Cam* cams, int V, const char* who) {
  SIU3R_CHECK(cams && V >= 1 && V <= 65535, "%s: bad view array (V = %d)", who, V);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK(cams[v].mode == 0 && cams[v].width == cams[0].width && cams[v].height == cams[0].height && cams[v].width > 0 && cams[v].height > 0,
                "%s: the backward covers the 3DGS family (mode 0) with one frame size per call", who);
  return 0;
}

}  // namespace

extern "C" int siu3r_raster_composite_rgb_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                              const void* entries, int64_t cap_e, const float* rec, const float* image, const float* depth,
                                              const float* alpha, const float* g_image, const float* g_depth, const float* g_alpha, float* grad,
                                              void* stream) {
  if (int rc = check_k2_views(cams_host, V, "raster_composite_rgb_bwd")) return rc;
  SIU3R_CHECK(cams_dev && bin_start && image && depth && alpha && g_image && g_depth && g_alpha && (G == 0 || (entries && rec && grad)),
              "raster_composite_rgb_bwd: null pointer");
  SIU3R_CHECK(G >= 0 && G < (1ll << 31) && cap_e > 0, "raster_composite_rgb_bwd: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) return 0;
  if (hipMemsetAsync(grad, 0, sizeof(float) * GR_N * (size_t)V * G, s) != hipSuccess) {
    siu3r_set_error("raster_composite_rgb_bwd: memset failed");
    return 2;
  }
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  hipLaunchKernelGGL(composite_rgb_bwd_kernel<false>, dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, bin_start, (const uint2*)entries, cap_e, rec, G,
                     image, depth, alpha, g_image, g_depth, g_alpha, grad);
  SIU3R_LAUNCH_CHECK("siu3r_raster_composite_rgb_bwd");
  return 0;
}

extern "C" int siu3r_raster_composite_rgb_bwd_k3(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                                 const void* entries, int64_t cap_e, const float* rec, const float* colors, const float* alphas,
                                                 const float* g_colors, const float* g_alphas, float* grad, void* stream) {
  SIU3R_CHECK(cams_host && V >= 1 && V <= 65535, "raster_composite_rgb_bwd_k3: bad view array (V = %d)", V);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK(cams_host[v].mode == 1 && cams_host[v].width == cams_host[0].width && cams_host[v].height == cams_host[0].height && cams_host[v].width > 0 &&
                    cams_host[v].height > 0,
                "raster_composite_rgb_bwd_k3: the gsplat family (mode 1) with one frame size per call");
  SIU3R_CHECK(cams_dev && bin_start && colors && alphas && g_colors && g_alphas && (G == 0 || (entries && rec && grad)), "raster_composite_rgb_bwd_k3: null pointer");
  SIU3R_CHECK(G >= 0 && G < (1ll << 31) && cap_e > 0, "raster_composite_rgb_bwd_k3: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) return 0;
  if (hipMemsetAsync(grad, 0, sizeof(float) * GR_N * (size_t)V * G, s) != hipSuccess) {
    siu3r_set_error("raster_composite_rgb_bwd_k3: memset failed");
    return 2;
  }
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  hipLaunchKernelGGL(composite_rgb_bwd_kernel<true>, dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, bin_start, (const uint2*)entries, cap_e, rec, G,
                     colors, (const float*)nullptr, alphas, g_colors, (const float*)nullptr, g_alphas, grad);
  SIU3R_LAUNCH_CHECK("siu3r_raster_composite_rgb_bwd_k3");
  return 0;
}

extern "C" int siu3r_raster_project_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                        int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect,
                                        const float* grad, float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d,
                                        float* pose_part, void* stream) {
  if (int rc = check_k2_views(cams_host, V, "raster_project_bwd")) return rc;
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "raster_project_bwd: G = %ld out of range", (long)G);
  SIU3R_CHECK(cams_dev && (G == 0 || (means && cov && opacities && colors && rect && grad && g_means && g_cov && g_opacities && g_colors)),
              "raster_project_bwd: null pointer");
  SIU3R_CHECK(cov_stride == 6 || cov_stride == 9, "raster_project_bwd: cov_stride must be 6 or 9");
  SIU3R_CHECK(!sh_planar || channels == 25, "raster_project_bwd: the planar SH layout needs 25 coefficients");
  SIU3R_CHECK(channels >= 1 && channels <= 25, "raster_project_bwd: 1 .. 25 colour coefficients (got %d)", channels);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK(cams_host[v].sh_degree < 0 ? (channels == 1 && !sh_planar) : channels >= (cams_host[v].sh_degree + 1) * (cams_host[v].sh_degree + 1),
                "raster_project_bwd: colour coefficients do not match sh_degree");
  if (G == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(project_bwd_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, s, (const Cam*)cams_dev, V, G, means, cov, cov_stride, opacities, colors,
                     channels, sh_planar, rect, grad, g_means, g_cov, g_opacities, g_colors, g_mean2d, pose_part);
  SIU3R_LAUNCH_CHECK("siu3r_raster_project_bwd");
  return 0;
}

extern "C" int64_t siu3r_raster_pose_partial_rows(int64_t G) { return G > 0 ? cdiv64(G, 256) : 0; }

extern "C" int siu3r_raster_pose_reduce(int V, int64_t nrows, const float* pose_part, float* g_pose, void* stream) {
  SIU3R_CHECK(V >= 1 && V <= 65535 && nrows >= 0 && g_pose && (nrows == 0 || pose_part), "raster_pose_reduce: bad arguments");
  hipLaunchKernelGGL(pose_reduce_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, V, nrows, pose_part, g_pose);
  SIU3R_LAUNCH_CHECK("siu3r_raster_pose_reduce");
  return 0;
}
