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
//                   (tile, Gaussian, term).  ABS (compile time, K2 only): the same walk also sums |mean x term| and |mean y term| per
//                   pixel (AbsGS, Ye et al. 2024: the densification signal that does not cancel over a Gaussian's footprint) through two
//                   more slots of the staged entry into abs_mean2d [V,G,2]; the signed record is formed exactly as without it.
//   projection bwd  one thread per Gaussian, looping over the call's views like project_kernel: per-Gaussian gradients are plain stores.
//                   The six pose terms of a view are summed per workgroup into a partial row; rows_reduce_kernel<6, 6> sums the rows.
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
// ABS (compile time): two more slots per staged entry, the wave sums of |gv[GR_MX]| and |gv[GR_MY]|, flushed into abs_mean2d [V,G,2].  Every
// addition is under `if constexpr`: the plain instantiations keep their registers, their LDS (row stride GR_N) and their code.
template <bool K3 = false, bool ABS = false>
__global__ __launch_bounds__(256) void composite_rgb_bwd_kernel(const Cam* __restrict__ cams, Geo geo, const int32_t* __restrict__ bin_start,
                                                                const uint2* __restrict__ entries, int64_t cap_e, const float* __restrict__ rec, int64_t G,
                                                                const float* __restrict__ image, const float* __restrict__ depth,
                                                                const float* __restrict__ alpha, const float* __restrict__ g_image,
                                                                const float* __restrict__ g_depth, const float* __restrict__ g_alpha,
                                                                float* __restrict__ grad, float* __restrict__ abs_mean2d) {
  constexpr int GS = ABS ? GR_N + 2 : GR_N;                     // slots per staged entry
  __shared__ __attribute__((aligned(16))) float s_a[BSTG][4];   // mx, my, depth, id
  __shared__ __attribute__((aligned(16))) float s_co[BSTG][4];  // conic a, b, c, opacity
  __shared__ __attribute__((aligned(16))) float s_c[BSTG][4];   // r, g, b
  __shared__ int s_m[BSTG];                                     // quadrant mask (the forward's)
  __shared__ float s_g[BSTG][GS];                               // the tile's summed gradient terms per staged entry (ABS: + |mx|, |my|)
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
      s_m[off] = quadrant_mask<K3>(r0, r1, alpha_min, tile_x0, tile_y0);  // the forward's: a wave skips exactly the entries the forward's wave skipped
#pragma unroll
      for (int k = 0; k < GS; ++k) s_g[off][k] = 0.f;
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
          if constexpr (ABS) {
            // the pixel's |mean terms|: 0 where it does not blend and where its alpha sits on the clamp, as the signed terms are
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const float av = fabsf(gv[k == 0 ? GR_MX : GR_MY]);
              if (__ballot(av != 0.f) == 0ull) continue;
              const float s = wave_sum(av);
              if (lane == 0 && s != 0.f) atomicAdd(&s_g[j][GR_N + k], s);
            }
          }
        }
        if (__ballot(!done) == 0ull) break;
      }
    }
    __syncthreads();
    // one global add per (tile, Gaussian, non-zero term): ten consecutive lanes cover one Gaussian's 40-byte row
    // (ABS: twelve lanes per Gaussian, the last two add into its 8-byte row of abs_mean2d)
    for (int q = t; q < n * GS; q += 256) {
      const int j = q / GS, k = q - j * GS;
      const float s = s_g[j][k];
      if constexpr (ABS) {
        const int64_t row = vg + __float_as_int(s_a[j][3]);
        if (s != 0.f) atomicAdd(k < GR_N ? &grad[row * GR_N + k] : &abs_mean2d[row * 2 + (k - GR_N)], s);
      } else {
        if (s != 0.f) atomicAdd(&grad[(vg + __float_as_int(s_a[j][3])) * GR_N + k], s);
      }
    }
  }
}

// ---- projection backward -----------------------------------------------------------------------------------------------------------
// grad [V, G, GR_N] (composite backward) -> g_means [G,3], g_cov [G, cov_stride], g_opac [G], g_colors (the layout of colors),
// g_mean2d [V, G, 2] (optional: the pixel-space mean gradient), pose_part [gridDim.x, V, 6] (optional: per-workgroup sums of
// d loss / d (rho, theta) of a left perturbation w2c <- exp(xi^) w2c).
// AA (compile time): the backward of project_kernel<true>, whose record opacity is opacity * comp, comp = sqrt(max(2.5e-5, r)), r = det0 / det
// (det0 = conic_det of the 2-D covariance before the dilation B, det = the dilated one's).  g_opac takes comp * grad[OP]; above the floor
// d loss / d comp = grad[OP] * opacity goes through d comp / d r = 0.5 / comp and, with det - det0 = B (c00' + c11' + B) used to cancel
// the leading terms by hand (the quotient rule's (c11' det - det0 c11) loses c00' / B digits on a large splat),
//   d r / d c00' = B (c11' c11 + c01^2) / det^2,  d r / d c11' = B (c00' c00 + c01^2) / det^2,  d r / d c01 = -2 c01 B (c00' + c11) / det^2
// (sums of like-signed terms) into the 2-D covariance gradient, next to the conic's, in front of the one chain (project_cov2d_bwd<true>).
// On the floor comp is a constant.
template <bool AA>
__global__ __launch_bounds__(256) void project_bwd_kernel(const Cam* __restrict__ cams, int V, int64_t G, const float* __restrict__ means,
                                                          const float* __restrict__ cov, int cov_stride, const float* __restrict__ opac,
                                                          const float* __restrict__ colors, int channels, int sh_planar,
                                                          const int32_t* __restrict__ rect, const float* __restrict__ grad, float* __restrict__ g_means,
                                                          float* __restrict__ g_cov, float* __restrict__ g_opac, float* __restrict__ g_colors,
                                                          float* __restrict__ g_mean2d, float* __restrict__ pose_part) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < G;
  float m[3] = {0.f, 0.f, 0.f}, S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool tri = cov_stride == 6;
  if (live) load_gaussian(means, cov, cov_stride, g, m, S);
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
      const Lens lens = lens_k2(c);
      const float fx = lens.fx, fy = lens.fy;
      const Cov2D p = project_cov2d(lens, W, tx, ty, tz, S);
      Cov2DGrad q;
      float cmp = 1.0f;
      if constexpr (AA) {
        // comp as the forward formed it (the same operations: the same bits, so the same side of the floor)
        const float c00p = p.a[0] * p.t0[0] + p.a[1] * p.t0[1] + p.a[2] * p.t0[2];
        const float c11p = p.b[0] * p.t1[0] + p.b[1] * p.t1[1] + p.b[2] * p.t1[2];
        const float r_ = conic_det(c00p, p.c01, c11p) / p.det;
        cmp = sqrtf(fmaxf(2.5e-5f, r_));
        float e00 = 0.f, e01 = 0.f, e11 = 0.f;
        if (r_ > 2.5e-5f) {
          const float rdet = 1.0f / p.det;
          const float dr = ((gr[GR_OP] * opac[g]) * (0.5f / cmp)) * ((lens.blur * rdet) * rdet);  // d loss / d r times B / det^2
          const float c01sq = p.c01 * p.c01;
          e00 = dr * (c11p * p.c11 + c01sq);
          e11 = dr * (c00p * p.c00 + c01sq);
          e01 = dr * (-2.0f * p.c01 * (c00p + p.c11));
        }
        q = project_cov2d_bwd<true>(p, W, gr[GR_CA], gr[GR_CB], gr[GR_CC], gS, e00, e01, e11);
      } else {
        q = project_cov2d_bwd(p, W, gr[GR_CA], gr[GR_CB], gr[GR_CC], gS);
      }
      const float W0[3] = {W[0], W[1], W[2]}, W1[3] = {W[4], W[5], W[6]}, W2[3] = {W[8], W[9], W[10]};
      // d loss / d W through the covariance only (rows), for the rotation part of the pose gradient
      float GW[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        GW[0][i] = p.j00 * q.dt0[i];
        GW[1][i] = p.j11 * q.dt1[i];
        GW[2][i] = p.j02 * q.dt0[i] + p.j12 * q.dt1[i];
      }
      // Jacobian -> camera-space point (the clamp of txz / tyz passes nothing to the clamped component)
      const float rz = p.rz;
      float drz = q.dj00 * fx + q.dj11 * fy - 2.0f * fx * p.ctx * rz * q.dj02 - 2.0f * fy * p.cty * rz * q.dj12;
      const float dctx = -fx * rz * rz * q.dj02, dcty = -fy * rz * rz * q.dj12;
      float dtz = dctx * p.cxz + dcty * p.cyz + gr[GR_Z];
      const float dtxz = (p.cxz == p.txz) ? dctx * tz : 0.f, dtyz = (p.cyz == p.tyz) ? dcty * tz : 0.f;
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
      if constexpr (AA) gop += cmp * gr[GR_OP];
      else gop += gr[GR_OP];
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
        const float3 gdm = sh_color_bwd(view_dir(m, c.campos), c.sh_degree, c.sh_band4 != 0, gcol, coef,
                                        [&](int k, int ch, float gv) { gsh[3 * k + ch] += gv; });
        gm[0] += gdm.x;
        gm[1] += gdm.y;
        gm[2] += gdm.z;
      }
    }
    // (uniform: every thread of the workgroup runs every view)
    if (pose_part) block_sum_row<6>(dpose, pose_part + ((int64_t)blockIdx.x * V + v) * 6);
  }
  if (!live) return;
  // (kept in the kernel, in this form: as a shared function the [3,3] branch compiles to narrower stores and measured 1.3 % slower)
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

// the launcher body of the composite backwards (K3: no depth; ABS: + abs_mean2d [V,G,2], zeroed here like grad)
template <bool K3, bool ABS = false>
int composite_rgb_bwd(const char* who, const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start, const void* entries,
                      int64_t cap_e, const float* rec, const float* image, const float* depth, const float* alpha, const float* g_image, const float* g_depth,
                      const float* g_alpha, float* grad, float* abs_mean2d, void* stream) {
  if (int rc = check_views(cams_host, V, K3 ? 1 : 0, who)) return rc;
  SIU3R_CHECK(cams_dev && bin_start && image && alpha && g_image && g_alpha && (K3 || (depth && g_depth)) &&
                  (G == 0 || (entries && rec && grad && (!ABS || abs_mean2d))),
              "%s: null pointer", who);
  SIU3R_CHECK(G >= 0 && G < (1ll << 31) && cap_e > 0, "%s: bad sizes", who);
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) return 0;
  if (hipMemsetAsync(grad, 0, sizeof(float) * GR_N * (size_t)V * G, s) != hipSuccess ||
      (ABS && hipMemsetAsync(abs_mean2d, 0, sizeof(float) * 2 * (size_t)V * G, s) != hipSuccess)) {
    siu3r_set_error("%s: memset failed", who);
    return 2;
  }
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  hipLaunchKernelGGL((composite_rgb_bwd_kernel<K3, ABS>), dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, bin_start, (const uint2*)entries, cap_e,
                     rec, G, image, depth, alpha, g_image, g_depth, g_alpha, grad, abs_mean2d);
  SIU3R_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace

extern "C" int siu3r_raster_composite_rgb_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                              const void* entries, int64_t cap_e, const float* rec, const float* image, const float* depth,
                                              const float* alpha, const float* g_image, const float* g_depth, const float* g_alpha, float* grad,
                                              void* stream) {
  return composite_rgb_bwd<false>("siu3r_raster_composite_rgb_bwd", cams_host, V, cams_dev, G, bin_start, entries, cap_e, rec, image, depth, alpha, g_image, g_depth,
                                  g_alpha, grad, nullptr, stream);
}

extern "C" int siu3r_raster_composite_rgb_bwd_abs(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                                  const void* entries, int64_t cap_e, const float* rec, const float* image, const float* depth,
                                                  const float* alpha, const float* g_image, const float* g_depth, const float* g_alpha, float* grad,
                                                  float* abs_mean2d, void* stream) {
  return composite_rgb_bwd<false, true>("siu3r_raster_composite_rgb_bwd_abs", cams_host, V, cams_dev, G, bin_start, entries, cap_e, rec, image, depth, alpha,
                                        g_image, g_depth, g_alpha, grad, abs_mean2d, stream);
}

extern "C" int siu3r_raster_composite_rgb_bwd_k3(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                                 const void* entries, int64_t cap_e, const float* rec, const float* colors, const float* alphas,
                                                 const float* g_colors, const float* g_alphas, float* grad, void* stream) {
  return composite_rgb_bwd<true>("siu3r_raster_composite_rgb_bwd_k3", cams_host, V, cams_dev, G, bin_start, entries, cap_e, rec, colors, nullptr, alphas, g_colors,
                                 nullptr, g_alphas, grad, nullptr, stream);
}

// the launcher body of the two projection backwards (AA: the anti-aliased record's)
template <bool AA>
static int project_bwd(const char* who, const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                       int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect, const float* grad,
                       float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d, float* pose_part, void* stream) {
  if (int rc = check_views(cams_host, V, 0, who)) return rc;
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "%s: G = %ld out of range", who, (long)G);
  SIU3R_CHECK(cams_dev && (G == 0 || (means && cov && opacities && colors && rect && grad && g_means && g_cov && g_opacities && g_colors)),
              "%s: null pointer", who);
  SIU3R_CHECK(cov_stride == 6 || cov_stride == 9, "%s: cov_stride must be 6 or 9", who);
  SIU3R_CHECK(!sh_planar || channels == 25, "%s: the planar SH layout needs 25 coefficients", who);
  SIU3R_CHECK(channels >= 1 && channels <= 25, "%s: 1 .. 25 colour coefficients (got %d)", who, channels);
  for (int v = 0; v < V; ++v)
    SIU3R_CHECK(cams_host[v].sh_degree < 0 ? (channels == 1 && !sh_planar) : channels >= (cams_host[v].sh_degree + 1) * (cams_host[v].sh_degree + 1),
                "%s: colour coefficients do not match sh_degree", who);
  if (G == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(project_bwd_kernel<AA>, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, s, (const Cam*)cams_dev, V, G, means, cov, cov_stride, opacities, colors,
                     channels, sh_planar, rect, grad, g_means, g_cov, g_opacities, g_colors, g_mean2d, pose_part);
  SIU3R_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int siu3r_raster_project_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                        int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect,
                                        const float* grad, float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d,
                                        float* pose_part, void* stream) {
  return project_bwd<false>("raster_project_bwd", cams_host, V, cams_dev, G, means, cov, cov_stride, opacities, colors, channels, sh_planar, rect, grad, g_means,
                            g_cov, g_opacities, g_colors, g_mean2d, pose_part, stream);
}

extern "C" int siu3r_raster_project_bwd_aa(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                           int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect,
                                           const float* grad, float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d,
                                           float* pose_part, void* stream) {
  return project_bwd<true>("raster_project_bwd_aa", cams_host, V, cams_dev, G, means, cov, cov_stride, opacities, colors, channels, sh_planar, rect, grad,
                           g_means, g_cov, g_opacities, g_colors, g_mean2d, pose_part, stream);
}

extern "C" int64_t siu3r_raster_pose_partial_rows(int64_t G) { return G > 0 ? cdiv64(G, 256) : 0; }

extern "C" int siu3r_raster_pose_reduce(int V, int64_t nrows, const float* pose_part, float* g_pose, void* stream) {
  SIU3R_CHECK(V >= 1 && V <= 65535 && nrows >= 0 && g_pose && (nrows == 0 || pose_part), "raster_pose_reduce: bad arguments");
  hipLaunchKernelGGL((rows_reduce_kernel<6, 6>), dim3(V), dim3(256), 0, (hipStream_t)stream, V, nrows, pose_part, g_pose);
  SIU3R_LAUNCH_CHECK("siu3r_raster_pose_reduce");
  return 0;
}
