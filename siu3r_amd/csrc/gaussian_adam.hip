// Fused visibility-aware Adam of splat refinement: ONE launch updates up to SIU3R_ADAM_MAX_FIELDS fields, each a dense
// fp32 [G, width] array with its gradient and its two moments, and leaves alone every row (Gaussian) that no view of the iteration's render
// saw.  The field table travels by value in the kernel arguments: no upload, no allocation, no host synchronisation.
//
// A visible row, in fp32 and in this operation order (torch.optim.Adam, amsgrad = False, no weight decay; -ffp-contract=off, correctly
// rounded divide and square root):
//   m = b1 * m + (1 - b1) * g;   v = b2 * v + ((1 - b2) * g) * g;   p = p - ((lr / bc1) * m) / (sqrt(v) / sqrt(bc2) + eps)
// 1 - b1 and 1 - b2 are formed in double from the caller's double betas and rounded once (1.f - (float)0.999 would be off by 1.3e-5 of
// itself, which is what torch avoids too); bc1 = 1 - b1^t and bc2 = 1 - b2^t come from the caller (computed in double).
// t is the optimiser's GLOBAL step count, also for a row that earlier steps skipped: a defined choice of this project.  The "sparse Adam"
// of the 3DGS code base was not available to compare with, so how it counts the steps of a skipped row is UNVERIFIED here.  Non-finite
// gradients propagate as in the float64 restatement (tests/dense_adam64.py); nothing is special-cased.
// lr of an element: its index within the row, i, steps with `lr` when head_period == 0 or i % head_period == 0, with `lr_tail` otherwise
// (harmonics [G,3,n] with head_period = n: the DC coefficient of each colour at lr, the higher bands at lr_tail).
// Visibility: a byte per row (the caller's mask, or the workspace that adam_visible_kernel fills from the K2 render's radii [V,G,R]: any
// entry > 0), or none at all.  An invisible row is not written and its gradient is not read.
// Work split: the elements of every field are cut into chunks of 1,024 floats; a workgroup (256 threads, 4 consecutive floats each, 16-byte
// accesses where the four bases of the field allow and the four elements are all visible, scalar accesses otherwise) takes chunks in a
// grid-stride loop over at most 2,048 workgroups.  Elementwise, no atomics: two calls on equal inputs give equal bits.  All element and
// row indices are 64-bit.
#include "block_reduce.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int PX = 4;            // floats per thread
constexpr int CHUNK = NT * PX;   // floats per workgroup and round
constexpr int MAXF = SIU3R_ADAM_MAX_FIELDS;
constexpr int MAX_GRID = 2048;   // 256 CUs x 8 workgroups

struct AdamArgs {
  siu3r_adam_field f[MAXF];
  int64_t chunk0[MAXF + 1];  // first chunk of field k; chunk0[n_fields] = all chunks
  int64_t G;
  const uint8_t* vis;        // [G] or null
  int n_fields;
  float b1, omb1, b2, omb2, eps, bc1, bc2;
};

__device__ inline void adam1(float& p, float g, float& m, float& v, float step, float b1, float omb1, float b2, float omb2, float bc2s, float eps) {
  m = b1 * m + omb1 * g;
  v = b2 * v + omb2 * g * g;
  p = p - step * m / (sqrtf(v) / bc2s + eps);
}

__global__ __launch_bounds__(NT) void gaussian_adam_kernel(AdamArgs a) {
  const float omb1 = a.omb1, omb2 = a.omb2, bc2s = sqrtf(a.bc2);
  const int64_t chunks = a.chunk0[a.n_fields];
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    int fi = 0;
#pragma unroll
    for (int k = 1; k < MAXF; ++k)
      if (k < a.n_fields && c >= a.chunk0[k]) fi = k;
    const siu3r_adam_field f = a.f[fi];
    const int64_t N = a.G * (int64_t)f.width;
    const int64_t e0 = (c - a.chunk0[fi]) * CHUNK + (int64_t)threadIdx.x * PX;
    if (e0 >= N) continue;
    // one decision per workgroup: a chunk starts a multiple of 4 KiB into the field, so only the four bases matter
    const bool vec = aligned16(f.param) && aligned16(f.grad) && aligned16(f.exp_avg) && aligned16(f.exp_avg_sq) && e0 + PX <= N;
    const uint32_t width = (uint32_t)f.width, hp = (uint32_t)f.head_period;
    int64_t row;
    uint32_t col;
    if (e0 <= 0xffffffffll) {  // (the 32-bit divide is several times cheaper, and almost every call fits)
      const uint32_t q = (uint32_t)e0 / width;
      row = q, col = (uint32_t)e0 - q * width;
    } else {
      row = e0 / (int64_t)width, col = (uint32_t)(e0 - row * (int64_t)width);
    }
    uint32_t hcol = hp ? col % hp : 0u;
    const float step_head = f.lr / a.bc1, step_tail = f.lr_tail / a.bc1;
    bool on[PX];
    float step[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      on[k] = e0 + k < N && (!a.vis || a.vis[row] != 0);
      step[k] = hp == 0u || hcol == 0u ? step_head : step_tail;
      ++col, ++hcol;
      if (hcol == hp) hcol = 0u;
      if (col == width) col = 0u, hcol = 0u, ++row;
    }
    if (vec && on[0] && on[1] && on[2] && on[3]) {
      float4 p = *reinterpret_cast<float4*>(f.param + e0), m = *reinterpret_cast<float4*>(f.exp_avg + e0), v = *reinterpret_cast<float4*>(f.exp_avg_sq + e0);
      const float4 g = *reinterpret_cast<const float4*>(f.grad + e0);
      adam1(p.x, g.x, m.x, v.x, step[0], a.b1, omb1, a.b2, omb2, bc2s, a.eps);
      adam1(p.y, g.y, m.y, v.y, step[1], a.b1, omb1, a.b2, omb2, bc2s, a.eps);
      adam1(p.z, g.z, m.z, v.z, step[2], a.b1, omb1, a.b2, omb2, bc2s, a.eps);
      adam1(p.w, g.w, m.w, v.w, step[3], a.b1, omb1, a.b2, omb2, bc2s, a.eps);
      *reinterpret_cast<float4*>(f.exp_avg + e0) = m;
      *reinterpret_cast<float4*>(f.exp_avg_sq + e0) = v;
      *reinterpret_cast<float4*>(f.param + e0) = p;
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        if (on[k]) {
          float p = f.param[e0 + k], m = f.exp_avg[e0 + k], v = f.exp_avg_sq[e0 + k];
          adam1(p, f.grad[e0 + k], m, v, step[k], a.b1, omb1, a.b2, omb2, bc2s, a.eps);
          f.exp_avg[e0 + k] = m;
          f.exp_avg_sq[e0 + k] = v;
          f.param[e0 + k] = p;
        }
      }
    }
  }
}

// vis[g] = any of radii[v, g, 0..R-1] > 0 over the views
__global__ __launch_bounds__(NT) void adam_visible_kernel(const int32_t* radii, int V, int64_t G, int R, uint8_t* vis) {
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < G; g += (int64_t)gridDim.x * NT) {
    bool seen = false;
    for (int v = 0; v < V; ++v) {
      const int32_t* r = radii + ((int64_t)v * G + g) * R;
      for (int k = 0; k < R; ++k) seen = seen || r[k] > 0;
    }
    vis[g] = seen ? 1 : 0;
  }
}

}  // namespace

extern "C" int64_t siu3r_gaussian_adam_ws(int64_t G) { return G > 0 ? (G + 15) / 16 * 16 : 0; }

extern "C" int siu3r_gaussian_adam(const siu3r_adam_field* fields, int n_fields, int64_t G, double beta1, double beta2, float eps, float bc1, float bc2,
                                   const int32_t* radii, int V, int R, const uint8_t* mask, void* ws, void* stream) {
  SIU3R_CHECK(fields, "gaussian_adam: null field table");
  SIU3R_CHECK(n_fields >= 1 && n_fields <= MAXF, "gaussian_adam: %d fields (1 .. %d)", n_fields, MAXF);
  SIU3R_CHECK(G > 0 && G <= ((int64_t)1 << 40), "gaussian_adam: %lld rows", (long long)G);
  SIU3R_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "gaussian_adam: betas (%g, %g) must lie in [0, 1)", beta1, beta2);
  SIU3R_CHECK(eps >= 0.f && bc1 > 0.f && bc1 <= 1.f && bc2 > 0.f && bc2 <= 1.f, "gaussian_adam: eps %g must be >= 0 and the bias corrections (%g, %g) in (0, 1]",
              (double)eps, (double)bc1, (double)bc2);
  SIU3R_CHECK(!(radii && mask), "gaussian_adam: radii and mask are two forms of one visibility, pass at most one");
  if (radii) {
    SIU3R_CHECK(V > 0 && R > 0, "gaussian_adam: radii [%d, G, %d] are empty", V, R);
    SIU3R_CHECK(ws, "gaussian_adam: radii need the workspace (siu3r_gaussian_adam_ws bytes)");
  }
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  a.chunk0[0] = 0;
  for (int k = 0; k < n_fields; ++k) {
    const siu3r_adam_field& f = fields[k];
    SIU3R_CHECK(f.param && f.grad && f.exp_avg && f.exp_avg_sq, "gaussian_adam: field %d has a null pointer", k);
    SIU3R_CHECK(f.width > 0, "gaussian_adam: field %d has width %d", k, f.width);
    SIU3R_CHECK(f.head_period >= 0, "gaussian_adam: field %d has head_period %d", k, f.head_period);
    SIU3R_CHECK(f.lr >= 0.f && f.lr_tail >= 0.f, "gaussian_adam: field %d has a negative or NaN learning rate (%g, %g)", k, (double)f.lr, (double)f.lr_tail);
    a.f[k] = f;
    a.chunk0[k + 1] = a.chunk0[k] + cdiv64(G * (int64_t)f.width, CHUNK);
  }
  a.G = G;
  a.n_fields = n_fields;
  a.b1 = (float)beta1, a.omb1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.omb2 = (float)(1.0 - beta2), a.eps = eps, a.bc1 = bc1, a.bc2 = bc2;
  a.vis = mask;
  hipStream_t s = (hipStream_t)stream;
  if (radii) {
    const int64_t blocks = cdiv64(G, NT);
    hipLaunchKernelGGL(adam_visible_kernel, dim3((unsigned)(blocks < MAX_GRID ? blocks : MAX_GRID)), dim3(NT), 0, s, radii, V, G, R, (uint8_t*)ws);
    SIU3R_LAUNCH_CHECK("siu3r_gaussian_adam (visibility)");
    a.vis = (const uint8_t*)ws;
  }
  const int64_t chunks = a.chunk0[n_fields];
  hipLaunchKernelGGL(gaussian_adam_kernel, dim3((unsigned)(chunks < MAX_GRID ? chunks : MAX_GRID)), dim3(NT), 0, s, a);
  SIU3R_LAUNCH_CHECK("siu3r_gaussian_adam");
  return 0;
}
