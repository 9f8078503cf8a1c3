// Backward pass of the gsplat-family rasterizer (gsplat.rasterization conventions, mode 1): the gradients of the N-channel colours and
// the alphas with respect to the per-(view, Gaussian) screen-space record, and from there to the Gaussians (means, covariances,
// opacities, features) and to every view's world->camera matrix; plus the backward passes of the two viewer helpers (quaternion + scale ->
// covariance, SH -> RGB).  The three-channel fused path's composite backward is composite_rgb_bwd_kernel<true> (raster_bwd.hip).
//
//   composite bwd   one wave per 8 x 8 quadrant, walking the quadrant's list (ql_build_kernel, raster_quad_lists.h) front to back in chunks of
//                   32 entries, with the forward's alpha / transmittance operations (composite_feat5_kernel):
//                     1. e[entry][pixel] = f_entry . G_pixel (G = upstream colour gradient) on the matrix cores: 32 x 64 per chunk, the
//                        channels as the reduction dimension; through the wave's LDS rows every lane (pixel) then holds the chunk's 32
//                        values of its own pixel;
//                     2. the scalar walk per lane = pixel: d loss / d alpha = T (e + g_alpha) - (behind) / (1 - alpha), with the part behind
//                        an entry = the saved totals (sum_c out G, alphas) minus the running prefix; the six screen-space terms go through
//                        wave sums, one float atomic per (quadrant, Gaussian, non-zero term);
//                     3. the weights w[pixel][entry] go through LDS (the transpose: A operand of the next product);
//                     4. d loss / d F[entry][channel] = sum_pixel w G on the matrix cores, one 32 x 32 block per 32 channels;
//                     5. added to g_feats [G, C] with global float atomics in the accumulator's own layout (per register: two entries x
//                        32 consecutive channels = two 128-byte row segments).
//                   The upstream gradient rows are re-read from L2 for both products (the operand choice).
//   projection bwd  one thread per Gaussian, looping over the views: per-Gaussian gradients are plain stores, the 12 terms of d loss / d
//                   [R | t] of a view are summed per workgroup into a partial row that rows_reduce_kernel<12, 16> sums.
// The gradient is that of the function the forward computes, on the branch it took: near / far culling, det <= 0, the radius and
// radius_clip, tile rects and list membership, the sigma < 0 skip, the alpha_min cut-off, saturation and the alpha_max clamp are held
// constant; the Jacobian clamp passes no gradient to the clamped component; a colour clamped at 0 passes none to its SH coefficients.
#include "common.h"
#include "gaussian_shared.h"
#include "raster_shared.h"
#include "raster_quad_lists.h"
#include "raster_bwd_shared.h"

namespace {

typedef siu3r_raster_cam Cam;
typedef float f32x16 __attribute__((ext_vector_type(16)));
struct __attribute__((packed, aligned(4))) f4u {  // 16 bytes at 4-byte alignment (rows of C floats: any C)
  float v[4];
};

// four consecutive floats of a row of n, zero beyond n (or everything when row is null)
__device__ __forceinline__ void load4(const float* row, int c, int n, float* o) {
  if (row && c + 3 < n) {
    const f4u t = *(const f4u*)(row + c);
    o[0] = t.v[0], o[1] = t.v[1], o[2] = t.v[2], o[3] = t.v[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (row && c + e < n) ? row[c + e] : 0.f;
  }
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---- N-channel composite backward ---------------------------------------------------------------------------------------------------
constexpr int QC = 32;  // list entries per chunk
__global__ __launch_bounds__(256) void composite_feat_bwd_kernel(const Cam* __restrict__ cams, Geo geo, const int32_t* __restrict__ tile_start,
                                                                 const int32_t* __restrict__ qids, const int32_t* __restrict__ qcnt, int64_t cap_d,
                                                                 const float* __restrict__ rec, const float* __restrict__ feats, int channels, int64_t G,
                                                                 const float* __restrict__ out, const float* __restrict__ out_alpha,
                                                                 const float* __restrict__ g_out, const float* __restrict__ g_alpha,
                                                                 float* __restrict__ grad, float* __restrict__ g_feats) {
  __shared__ __attribute__((aligned(16))) float s_rec[4][QC][8];  // per wave: {mx, my, 0, id | conic a, b, c, opacity}
  __shared__ float s_w[4][64][QC + 1];                            // per wave: blending weights [pixel][entry] (odd stride: no bank conflicts)
  const int v = blockIdx.y;
  const Cam& c = cams[v];
  const int tile = blockIdx.x, tx = tile % geo.gw, ty = tile / geo.gw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qx0 = tx * TILE + (wave & 1) * 8, qy0 = ty * TILE + (wave >> 1) * 8;
  const int width = c.width, height = c.height;
  const size_t hw = (size_t)width * height;
  const int C = channels;
  // rows of the upstream gradient: this lane's pixel (the walk), and pixel (lane & 31) of each 32-pixel block (B operand of the e product)
  auto grow = [&](int p) -> const float* {
    const int x = qx0 + (p & 7), y = qy0 + (p >> 3);
    return (x < width && y < height) ? g_out + ((size_t)v * hw + (size_t)y * width + x) * C : nullptr;
  };
  const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
  const bool inside = px < width && py < height;
  const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f;
  const float* gb0 = grow(lane & 31);
  const float* gb1 = grow(32 + (lane & 31));
  // the saved totals of this pixel: D = sum_c out G, alphas; the upstream alpha gradient
  float tD = 0.f, tO = 0.f, gO = 0.f;
  bool anyg = false;
  if (inside) {
    const size_t pix = (size_t)v * hw + (size_t)py * width + px;
    const float* orow = out + pix * C;
    const float* grw = g_out + pix * C;
    for (int ch = 0; ch < C; ch += 4) {
      float o4[4], g4[4];
      load4(orow, ch, C, o4);
      load4(grw, ch, C, g4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        tD += o4[e] * g4[e];
        anyg = anyg || g4[e] != 0.f;
      }
    }
    tO = out_alpha[pix];
    gO = g_alpha[pix];
    anyg = anyg || gO != 0.f;
  }
  const int32_t* ts = tile_start + (int64_t)v * (geo.T + 2);
  const int beg = ts[tile], len = ts[tile + 1] - beg;
  const int n = __builtin_amdgcn_readfirstlane(qcnt[((int64_t)v * geo.T + tile) * 4 + wave]);
  const int32_t* ql = qids + (int64_t)v * 4 * cap_d + 4 * (int64_t)beg + (int64_t)wave * len;
  const int64_t vg = (int64_t)v * G;
  const float alpha_min = c.alpha_min, alpha_max = c.alpha_max, t_min = c.t_min;
  float T = 1.0f, O = 0.f, S = 0.f;  // transmittance, alpha prefix, prefix of sum w e
  // a pixel with no upstream gradient contributes nothing: it leaves the walk at once (the other pixels' chains do not depend on it)
  bool done = !inside || !anyg;
  float (*sw)[QC + 1] = s_w[wave];
  for (int k0 = 0; k0 < n; k0 += QC) {
    if (__ballot(!done) == 0ull) break;
    // the chunk's ids and records (lanes 0..31; entries beyond the list: Gaussian 0, never blended)
    const int idv = (lane < QC && k0 + lane < n) ? ql[k0 + lane] : 0;
    if (lane < QC) {
      const float4* rp = (const float4*)(rec + 12 * (vg + idv));
      const float4 r0 = rp[0], r1 = rp[1];
      *(float4*)&s_rec[wave][lane][0] = make_float4(r0.x, r0.y, 0.f, __int_as_float(idv));
      *(float4*)&s_rec[wave][lane][4] = r1;
    }
    // 1. e[entry][pixel] over the channels: A = feature rows (entry = lane & 31), B = gradient rows (pixel = lane & 31 of block 0 / 1); a lane
    //    contributes channels ch + 4 * (lane >> 5) + q at reduction index lane >> 5 of MFMA q (the pairing only has to match between A and B)
    const float* frow = feats + (size_t)__shfl(idv, lane & 31) * C;
    f32x16 e0, e1;
#pragma unroll
    for (int r = 0; r < 16; ++r) e0[r] = 0.f, e1[r] = 0.f;
    for (int ch = 0; ch < C; ch += 8) {
      const int cc = ch + 4 * (lane >> 5);
      float a4[4], b0[4], b1[4];
      load4(frow, cc, C, a4);
      load4(gb0, cc, C, b0);
      load4(gb1, cc, C, b1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        e0 = mfma(a4[q], b0[q], e0);
        e1 = mfma(a4[q], b1[q], e1);
      }
    }
    // C/D layout: column (pixel of the block) = lane & 31, row (entry) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  Through the wave's LDS
    // rows (the weights' transpose buffer, free until the walk writes them): every lane reads the chunk's 32 values of its own pixel.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      sw[lane & 31][i] = e0[r];
      sw[32 + (lane & 31)][i] = e1[r];
    }
    float ev[QC];
#pragma unroll
    for (int i = 0; i < QC; ++i) ev[i] = sw[lane][i];
    // 2. the walk (the forward's operations in the forward's order, composite_feat5_kernel)
    bool any_w = false;
#pragma unroll
    for (int i = 0; i < QC; ++i) {
      const float e = ev[i];
      const float4 A = *(const float4*)&s_rec[wave][i][0], Q = *(const float4*)&s_rec[wave][i][4];
      const float dx = A.x - pxf, dy = A.y - pyf;
      const float sigma = conic_sigma(Q.x, Q.y, Q.z, dx, dy);
      const float ex = exp_det_sel(-sigma);
      const float a = fminf(alpha_max, Q.w * ex);
      const float nT = __builtin_fmaf(-T, a, T);
      const bool reach = !done && k0 + i < n && sigma >= 0.0f && a >= alpha_min;
      const bool sat = reach && nT <= t_min;
      done = done || sat;
      const bool ok = reach && !sat;
      float gv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float w = 0.f;
      if (ok) {
        w = a * T;
        O += w;
        S += w * e;
        // d loss / d alpha = T (e + g_alpha) - (everything behind this entry) / (1 - alpha)
        const float behind = (tD - S) + gO * (tO - O);
        const float dLda = T * (e + gO) - behind / (1.0f - a);
        if (!(Q.w * ex > alpha_max)) {  // alpha clamped at alpha_max: constant
          gv[GR_OP] = dLda * ex;
          const float dLdp = -dLda * a;  // d loss / d sigma
          gv[GR_CA] = 0.5f * dx * dx * dLdp;
          gv[GR_CC] = 0.5f * dy * dy * dLdp;
          gv[GR_CB] = dx * dy * dLdp;
          gv[GR_MX] = dLdp * (Q.x * dx + Q.y * dy);
          gv[GR_MY] = dLdp * (Q.z * dy + Q.y * dx);
        }
        T = nT;
      }
      sw[lane][i] = w;
      if (__ballot(ok) != 0ull) {
        any_w = true;
        const int id = __float_as_int(A.w);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
          // a term that is zero on the whole wave (alpha clamped, no gradient here) skips its sum
          if (__ballot(gv[t] != 0.f) == 0ull) continue;
          const float s = wave_sum(gv[t]);
          if (lane == 0 && s != 0.f) atomicAdd(&grad[(vg + id) * GR_N + t], s);
        }
      }
    }
    if (!any_w) continue;  // (uniform) no entry of the chunk blends into this quadrant: no feature gradient
    // 3.-5. d loss / d F[entry][channel] = sum over pixel pairs of w[entry][pixel] G[pixel][channel], 32 channels per accumulator block
    const int pl = lane >> 5;  // reduction index: pixel 2 m + pl of MFMA m
    for (int c0 = 0; c0 < C; c0 += 32) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int chn = c0 + (lane & 31);
#pragma unroll 4
      for (int m = 0; m < 32; ++m) {
        const float aw = sw[2 * m + pl][lane & 31];
        if (__ballot(aw != 0.f) == 0ull) continue;  // neither pixel of the pair blends an entry of the chunk
        const float* gr = grow(2 * m + pl);
        const float bg = (gr && chn < C) ? gr[chn] : 0.f;
        acc = mfma(aw, bg, acc);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * pl;
        const int id = __float_as_int(s_rec[wave][i][3]);
        if (k0 + i < n && chn < C && acc[r] != 0.f) atomicAdd(&g_feats[(size_t)id * C + chn], acc[r]);
      }
    }
  }
}

// ---- projection backward (mode 1) -------------------------------------------------------------------------------------------------
// grad [V, G, GR_N] -> g_means [G,3], g_cov [G, cov_stride], g_opac [G], g_colors [G,3] (optional: the three-channel path's colours from the
// record), pose_part [gridDim.x, V, 12] (optional: per-workgroup sums of d loss / d [R | t] of each view's world->camera matrix).
__global__ __launch_bounds__(256) void project_bwd_k3_kernel(const Cam* __restrict__ cams, int V, int64_t G, const float* __restrict__ means,
                                                             const float* __restrict__ cov, int cov_stride, const int32_t* __restrict__ rect,
                                                             const float* __restrict__ grad, float* __restrict__ g_means, float* __restrict__ g_cov,
                                                             float* __restrict__ g_opac, float* __restrict__ g_colors, float* __restrict__ pose_part) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < G;
  float m[3] = {0.f, 0.f, 0.f}, S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool tri = cov_stride == 6;
  if (live) load_gaussian(means, cov, cov_stride, g, m, S);
  float gm[3] = {0.f, 0.f, 0.f}, gS[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gop = 0.f, gcol[3] = {0.f, 0.f, 0.f};
  for (int v = 0; v < V; ++v) {
    const Cam& c = cams[v];
    float dW[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) dW[k] = 0.f;
    const int64_t o = (int64_t)v * G + g;
    const int4 r = live ? *(const int4*)(rect + 4 * o) : make_int4(0, 0, 0, 0);
    if (live && (r.z - r.x) * (r.w - r.y) != 0) {
      float gr[GR_N];
#pragma unroll
      for (int k = 0; k < GR_N; ++k) gr[k] = grad[o * GR_N + k];
      const float* W = c.w2c;
      const float tx = W[0] * m[0] + W[1] * m[1] + W[2] * m[2] + W[3];
      const float ty = W[4] * m[0] + W[5] * m[1] + W[6] * m[2] + W[7];
      const float tz = W[8] * m[0] + W[9] * m[1] + W[10] * m[2] + W[11];
      const Lens lens = lens_k3(c);
      const float fx = lens.fx, fy = lens.fy;
      const Cov2D p = project_cov2d(lens, W, tx, ty, tz, S);
      const Cov2DGrad q = project_cov2d_bwd(p, W, gr[GR_CA], gr[GR_CB], gr[GR_CC], gS);
      const float W0[3] = {W[0], W[1], W[2]}, W1[3] = {W[4], W[5], W[6]}, W2[3] = {W[8], W[9], W[10]};
      // Jacobian -> camera-space point (the clamp of txz / tyz passes nothing to the clamped component); mean2d = (fx txz + cx, fy tyz + cy)
      const float rz = p.rz;
      float drz = q.dj00 * fx + q.dj11 * fy - 2.0f * fx * p.ctx * rz * q.dj02 - 2.0f * fy * p.cty * rz * q.dj12;
      const float dctx = -fx * rz * rz * q.dj02, dcty = -fy * rz * rz * q.dj12;
      float dtz = dctx * p.cxz + dcty * p.cyz;
      const float dtxz = ((p.cxz == p.txz) ? dctx * tz : 0.f) + fx * gr[GR_MX], dtyz = ((p.cyz == p.tyz) ? dcty * tz : 0.f) + fy * gr[GR_MY];
      const float dtx = dtxz * rz, dty = dtyz * rz;
      drz += dtxz * tx + dtyz * ty;
      dtz += -drz * rz * rz;
      const float dp[3] = {dtx, dty, dtz};
#pragma unroll
      for (int i = 0; i < 3; ++i) gm[i] += W0[i] * dp[0] + W1[i] * dp[1] + W2[i] * dp[2];
      gop += gr[GR_OP];
      gcol[0] += gr[GR_R];
      gcol[1] += gr[GR_G];
      gcol[2] += gr[GR_B];
      if (pose_part) {
        // d loss / d R = (through the covariance: rows of M = J R) + dp m^T;  d loss / d t = dp
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          dW[i] = p.j00 * q.dt0[i] + dp[0] * m[i];
          dW[4 + i] = p.j11 * q.dt1[i] + dp[1] * m[i];
          dW[8 + i] = p.j02 * q.dt0[i] + p.j12 * q.dt1[i] + dp[2] * m[i];
        }
        dW[3] = dp[0], dW[7] = dp[1], dW[11] = dp[2];
      }
    }
    // (uniform: every thread of the workgroup runs every view)
    if (pose_part) block_sum_row<12>(dW, pose_part + ((int64_t)blockIdx.x * V + v) * 12);
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
  if (g_colors) {
    g_colors[3 * g] = gcol[0];
    g_colors[3 * g + 1] = gcol[1];
    g_colors[3 * g + 2] = gcol[2];
  }
}

// ---- quaternion + scale -> covariance backward (quat_scale_cov6_kernel, raster.hip) ---------------------------------------------------
// cov = M M^T, M = R(q / |q|) diag(s); g_cov6 [G,6] (upper triangle) -> g_quats [G,4] (w,x,y,z, through the normalisation), g_scales [G,3]
__global__ void quat_scale_cov6_bwd_kernel(int64_t G, const float* __restrict__ quats, const float* __restrict__ scales, const float* __restrict__ g_cov6,
                                           float* __restrict__ g_quats, float* __restrict__ g_scales) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const float4 q = *(const float4*)(quats + 4 * g);
  float R[9];
  const float inv = quat_rotation(q.x, q.y, q.z, q.w, R);
  const float w = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
  const float s[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
  float M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * r + j] = R[3 * r + j] * s[j];
  // symmetric gradient of cov from its six upper entries (xx, xy, xz, yy, yz, zz): cov[r][c] = M_r . M_c
  const float* gc = g_cov6 + 6 * g;
  const float Gs[9] = {gc[0], gc[1], gc[2], gc[1], gc[3], gc[4], gc[2], gc[4], gc[5]};
  float gM[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      // d/dM[r][j] of sum_{a<=b} g_ab M_a . M_b: diagonal 2 g_rr M_r, off-diagonal g_rb M_b
      float acc = 0.f;
#pragma unroll
      for (int b = 0; b < 3; ++b) acc += (b == r ? 2.0f : 1.0f) * Gs[3 * r + b] * M[3 * b + j];
      gM[3 * r + j] = acc;
    }
  float gR[9], gs[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gR[3 * r + j] = gM[3 * r + j] * s[j];
      gs[j] += gM[3 * r + j] * R[3 * r + j];
    }
  const float gw = 2.0f * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
  const float gx = 2.0f * (y * gR[1] + z * gR[2] + y * gR[3] - 2.0f * x * gR[4] - w * gR[5] + z * gR[6] + w * gR[7] - 2.0f * x * gR[8]);
  const float gy = 2.0f * (-2.0f * y * gR[0] + x * gR[1] + w * gR[2] + x * gR[3] + z * gR[5] - w * gR[6] + z * gR[7] - 2.0f * y * gR[8]);
  const float gz = 2.0f * (-2.0f * z * gR[0] - w * gR[1] + x * gR[2] + w * gR[3] - 2.0f * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
  // through q / |q|: (g - n (n . g)) / |q|
  const float dd = gw * w + gx * x + gy * y + gz * z;
  g_quats[4 * g] = (gw - w * dd) * inv;
  g_quats[4 * g + 1] = (gx - x * dd) * inv;
  g_quats[4 * g + 2] = (gy - y * dd) * inv;
  g_quats[4 * g + 3] = (gz - z * dd) * inv;
  g_scales[3 * g] = gs[0];
  g_scales[3 * g + 1] = gs[1];
  g_scales[3 * g + 2] = gs[2];
}

// ---- SH -> RGB backward (sh_eval_kernel, raster.hip) --------------------------------------------------------------------------------
// rgb = max(sum_k B_k(d) sh[k] + 0.5, 0), d = (m - campos) / |m - campos|.  g_rgb [G,3] -> g_sh [G,ncoef,3] (coefficients past the degree:
// 0), g_means [G,3] (written), g_campos [3] (added: one atomic triple per workgroup; zeroed by the launcher)
__global__ __launch_bounds__(256) void sh_eval_bwd_kernel(int64_t G, int ncoef, int degree, const float* __restrict__ means, const float* __restrict__ campos,
                                                          const float* __restrict__ sh, const float* __restrict__ g_rgb, float* __restrict__ g_sh,
                                                          float* __restrict__ g_means, float* __restrict__ g_campos) {
  __shared__ float s_c[4][3];
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float gmv[3] = {0.f, 0.f, 0.f};
  if (g < G) {
    const float* shp = sh + (size_t)g * ncoef * 3;
    float* gsp = g_sh + (size_t)g * ncoef * 3;
    for (int k = (degree + 1) * (degree + 1); k < ncoef; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gsp[3 * k + ch] = 0.f;
    const float gcol[3] = {g_rgb[3 * g], g_rgb[3 * g + 1], g_rgb[3 * g + 2]};
    const float3 gdm = sh_color_bwd(view_dir(means + 3 * g, campos), degree, true, gcol, [&](int k, int ch) { return shp[3 * k + ch]; },
                                    [&](int k, int ch, float gv) { gsp[3 * k + ch] = gv; });
    g_means[3 * g] = gmv[0] = gdm.x;
    g_means[3 * g + 1] = gmv[1] = gdm.y;
    g_means[3 * g + 2] = gmv[2] = gdm.z;
  }
  // the camera centre moves the direction the other way
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float s = wave_sum(gmv[k]);
    if (lane == 0) s_c[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const float s = s_c[0][k] + s_c[1][k] + s_c[2][k] + s_c[3][k];
    if (s != 0.f) atomicAdd(&g_campos[k], -s);
  }
}

}  // namespace

extern "C" int siu3r_raster_quad_lists(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start,
                                       const int32_t* ids, int64_t cap_d, const float* rec, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = check_views(cams_host, V, 1, "raster_quad_lists")) return rc;
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  SIU3R_CHECK(cams_dev && tile_start && (ids || cap_d == 0 || G == 0) && (rec || G == 0) && ws && (((uintptr_t)ws) & 3) == 0, "raster_quad_lists: bad arguments");
  SIU3R_CHECK(cap_d > 0 && cap_d < (1ll << 31) && ws_bytes >= (int64_t)V * (16 * cap_d + 16 * (int64_t)geo.T), "raster_quad_lists: workspace too small");
  int32_t* qids = (int32_t*)ws;
  int32_t* qcnt = qids + (int64_t)V * 4 * cap_d;
  hipLaunchKernelGGL(ql_build_kernel, dim3(geo.T, V), dim3(256), 0, (hipStream_t)stream, (const Cam*)cams_dev, geo, tile_start, ids, cap_d, rec, G, qids, qcnt);
  SIU3R_LAUNCH_CHECK("siu3r_raster_quad_lists");
  return 0;
}

extern "C" int siu3r_raster_composite_feat_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start,
                                               const void* ws, int64_t cap_d, const float* rec, const float* feats, int channels, const float* out,
                                               const float* out_alpha, const float* g_out, const float* g_alpha, float* grad, float* g_feats,
                                               void* stream) {
  if (int rc = check_views(cams_host, V, 1, "raster_composite_feat_bwd")) return rc;
  SIU3R_CHECK(cams_dev && tile_start && ws && out && out_alpha && g_out && g_alpha && (G == 0 || (rec && feats && grad && g_feats)),
              "raster_composite_feat_bwd: null pointer");
  SIU3R_CHECK(G >= 0 && G < (1ll << 31) && channels >= 1 && cap_d > 0 && cap_d < (1ll << 31) && (int64_t)G * channels < (1ll << 40),
              "raster_composite_feat_bwd: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) return 0;
  if (hipMemsetAsync(grad, 0, sizeof(float) * GR_N * (size_t)V * G, s) != hipSuccess ||
      hipMemsetAsync(g_feats, 0, sizeof(float) * (size_t)G * channels, s) != hipSuccess) {
    siu3r_set_error("raster_composite_feat_bwd: memset failed");
    return 2;
  }
  const Geo geo = make_geo(cams_host[0].width, cams_host[0].height);
  const int32_t* qids = (const int32_t*)ws;
  const int32_t* qcnt = qids + (int64_t)V * 4 * cap_d;
  hipLaunchKernelGGL(composite_feat_bwd_kernel, dim3(geo.T, V), dim3(256), 0, s, (const Cam*)cams_dev, geo, tile_start, qids, qcnt, cap_d, rec, feats, channels,
                     G, out, out_alpha, g_out, g_alpha, grad, g_feats);
  SIU3R_LAUNCH_CHECK("siu3r_raster_composite_feat_bwd");
  return 0;
}

extern "C" int siu3r_raster_project_bwd_k3(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                           int cov_stride, const int32_t* rect, const float* grad, float* g_means, float* g_cov, float* g_opacities,
                                           float* g_colors, float* pose_part, void* stream) {
  if (int rc = check_views(cams_host, V, 1, "raster_project_bwd_k3")) return rc;
  SIU3R_CHECK(G >= 0 && G < (1ll << 31), "raster_project_bwd_k3: G = %ld out of range", (long)G);
  SIU3R_CHECK(cams_dev && (G == 0 || (means && cov && rect && grad && g_means && g_cov && g_opacities)), "raster_project_bwd_k3: null pointer");
  SIU3R_CHECK(cov_stride == 6 || cov_stride == 9, "raster_project_bwd_k3: cov_stride must be 6 or 9");
  if (G == 0) return 0;
  hipLaunchKernelGGL(project_bwd_k3_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, (hipStream_t)stream, (const Cam*)cams_dev, V, G, means, cov, cov_stride,
                     rect, grad, g_means, g_cov, g_opacities, g_colors, pose_part);
  SIU3R_LAUNCH_CHECK("siu3r_raster_project_bwd_k3");
  return 0;
}

extern "C" int siu3r_raster_viewmat_reduce(int V, int64_t nrows, const float* pose_part, float* g_viewmats, void* stream) {
  SIU3R_CHECK(V >= 1 && V <= 65535 && nrows >= 0 && g_viewmats && (nrows == 0 || pose_part), "raster_viewmat_reduce: bad arguments");
  hipLaunchKernelGGL((rows_reduce_kernel<12, 16>), dim3(V), dim3(256), 0, (hipStream_t)stream, V, nrows, pose_part, g_viewmats);
  SIU3R_LAUNCH_CHECK("siu3r_raster_viewmat_reduce");
  return 0;
}

extern "C" int siu3r_quat_scale_to_cov6_bwd(const float* quats_wxyz, const float* scales, const float* g_cov6, float* g_quats, float* g_scales, int64_t G,
                                            void* stream) {
  SIU3R_CHECK(G >= 0 && (G == 0 || (quats_wxyz && scales && g_cov6 && g_quats && g_scales)), "quat_scale_to_cov6_bwd: null pointer");
  SIU3R_CHECK(((uintptr_t)quats_wxyz & 15) == 0, "quat_scale_to_cov6_bwd: quats must be 16-byte aligned");
  if (G > 0)
    hipLaunchKernelGGL(quat_scale_cov6_bwd_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, (hipStream_t)stream, G, quats_wxyz, scales, g_cov6, g_quats,
                       g_scales);
  SIU3R_LAUNCH_CHECK("siu3r_quat_scale_to_cov6_bwd");
  return 0;
}

extern "C" int siu3r_sh_eval_bwd(const float* means, const float* campos3_dev, const float* sh, int ncoef, int degree, const float* g_rgb, float* g_sh,
                                 float* g_means, float* g_campos3, int64_t G, void* stream) {
  SIU3R_CHECK(G >= 0 && campos3_dev && g_campos3 && (G == 0 || (means && sh && g_rgb && g_sh && g_means)), "sh_eval_bwd: null pointer");
  SIU3R_CHECK(degree >= 0 && degree <= 4 && ncoef >= (degree + 1) * (degree + 1), "sh_eval_bwd: degree %d needs %d coefficients, got %d", degree,
              (degree + 1) * (degree + 1), ncoef);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(g_campos3, 0, 3 * sizeof(float), s) != hipSuccess) {
    siu3r_set_error("sh_eval_bwd: memset failed");
    return 2;
  }
  if (G > 0)
    hipLaunchKernelGGL(sh_eval_bwd_kernel, dim3((unsigned)cdiv64(G, 256)), dim3(256), 0, s, G, ncoef, degree, means, campos3_dev, sh, g_rgb, g_sh, g_means,
                       g_campos3);
  SIU3R_LAUNCH_CHECK("siu3r_sh_eval_bwd");
  return 0;
}
