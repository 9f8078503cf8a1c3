// The row chain that ends every Mask2Former pixel-decoder encoder layer (reference video_seg_decoder.py:945-1018: output_proj + residual,
// self_attn_layer_norm, fc1 + ReLU, fc2 + residual, final_layer_norm) as ONE launch, bf16x3, d_model = 256:
//   y = x Wo^T + bo + res;  z = LN(y; g1, b1);  h = relu(z W1^T + c1);  o = h W2^T + c2 + z;  out = LN(o; g2, b2).
// Every step is row-local, so a workgroup owns 64 rows from the first load to the last store: the [M, H] hidden activation and four
// round trips of the [M, 256] residual stream never reach memory, and the two LayerNorms stop being launches.
//
// Workgroup = 8 waves x 64 rows.  Wave w owns output columns [32 w, 32 w + 32) of all 64 rows (two 32 x 32 accumulators) in every
// product.  The A operand of a product lives in LDS as hi / lo bf16 planes (padded rows, as proj.hip): s_a holds the split of x, then of
// z; s_h holds the split of one 256-column chunk of h.  fc2's accumulators stay in registers across the H / 256 chunks, z stays in the
// owning wave's accumulator-layout registers for the residual.  The weights are pre-split MFMA B fragments (ops.pack_proj's layout)
// that every wave streams from L2 as 16-byte pieces, one group of four K steps (eight pieces) ahead of the MFMAs that use them, across
// the pass boundaries too.  A LayerNorm goes through LDS as fp32 (the s_h bytes, free at those points): the owning waves write their
// columns, then wave w normalises rows 8 w .. 8 w + 7 with the lane -> column map, the sums and the butterfly of layernorm_kernel
// (elementwise.hip) -- the same bits for the same input -- and writes the planes of z (or the result rows) 4 columns per lane.
// Same products as siu3r_gemm (A_hi W_hi + A_lo W_hi + A_hi W_lo, A split by truncation), another K order.  No atomics, no split-K.
#include "common.h"

namespace {

constexpr int RC_D = 256;                           // d_model
constexpr int RC_ROWS = 64;                         // rows per workgroup
constexpr int RC_LD = RC_D + 8;                     // bf16 elements per staged plane row (16-byte aligned, spreads the banks)
constexpr int RC_PLANE = RC_ROWS * RC_LD + 32;      // + 64 bytes: the lo plane starts 16 banks after the hi plane (paired 4-byte stores)
constexpr int RC_LDF = RC_D + 4;                    // floats per row of the fp32 LayerNorm staging
static_assert(2 * RC_PLANE * 2 >= RC_ROWS * RC_LDF * 4, "the fp32 staging overlays the hidden chunk's planes");

struct RowchainParams {
  const float *x, *res;
  const uint4 *wo, *w1, *w2;  // fragments [NB][K / 16][2 planes][64 lanes] x 8 bf16
  const float *bo, *g1, *b1, *c2, *g2, *b2, *c1;
  float* out;
  int64_t M;
  int H;
  float eps1, eps2;
};

__device__ __forceinline__ void rc_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float rc_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void rc_load_w(uint4 (&wb)[8], const uint4* src) {
#pragma unroll
  for (int j = 0; j < 8; ++j) wb[j] = src[(j >> 1) * 128 + (j & 1) * 64];  // K step j / 2, plane j % 2
}

// One 256-deep pass of a wave: acc[b] += A[32 b .. 32 b + 31, 0 .. 255] W^T over its 32 columns.  a_hi / a_lo: the planes at the lane's
// fragment origin (row lane % 32, k 8 (lane / 32)); w: the pass's 16 K steps of fragments (+ lane); wb holds the first group of four
// K steps on entry and the first group of `w_next` (the next pass) on return.
__device__ __forceinline__ void rc_pass(const u16* a_hi, const u16* a_lo, const uint4* w, const uint4* w_next, uint4 (&wb)[8], f32x16 (&acc)[2]) {
  uint4 a[4], an[4];
  auto load_a = [&](uint4 (&d)[4], int ks) {
    d[0] = *(const uint4*)(a_hi + 16 * ks);
    d[1] = *(const uint4*)(a_lo + 16 * ks);
    d[2] = *(const uint4*)(a_hi + 32 * RC_LD + 16 * ks);
    d[3] = *(const uint4*)(a_lo + 32 * RC_LD + 16 * ks);
  };
  load_a(a, 0);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint4 wn[8];
    rc_load_w(wn, g < 3 ? w + (g + 1) * 4 * 128 : w_next);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ks = 4 * g + s;
      if (ks < 15) load_a(an, ks + 1);
      const bf16x8 bh = as_bf16x8(wb[2 * s]), bl = as_bf16x8(wb[2 * s + 1]);
      // per K step hi x hi, hi x lo, lo x hi: the order of the ping-pong GEMM (gemm_pp_kernel.h), whose launches this kernel replaces --
      // with the same operand bits in the same MFMA slots the accumulators are the GEMM's, bit for bit
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[0]), bh, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[2]), bh, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[0]), bl, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[2]), bl, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[1]), bh, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[3]), bh, acc[1], 0, 0, 0);
      if (ks < 15) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = an[i];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) wb[j] = wn[j];
  }
}

// LayerNorm of rows 8 wave .. 8 wave + 7 of the fp32 staging `f` (lane: columns 4 lane .. 4 lane + 3, as layernorm_kernel at C = 256).
// FINAL: the result goes to out (rows below M); else it replaces the row in `f` and its hi / lo planes go to s_hi / s_lo.
template <bool FINAL>
__device__ __forceinline__ void rc_layernorm(float* f, u16* s_hi, u16* s_lo, const float* gamma, const float* beta, float eps, float* out,
                                             int64_t row0, int64_t M, int wave, int lane) {
  const float4 g = *(const float4*)(gamma + 4 * lane), bb = *(const float4*)(beta + 4 * lane);
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) {
    const int r = 8 * wave + rr;
    float* fr = f + r * RC_LDF + 4 * lane;
    const float4 v = *(const float4*)fr;
    float sum = 0.f;
    sum += v.x + v.y + v.z + v.w;
    const float mean = rc_wave_sum(sum) / (float)RC_D;
    const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
    float sq = 0.f;
    sq += a * a + b * b + cc * cc + d * d;
    const float rstd = rsqrtf(rc_wave_sum(sq) / (float)RC_D + eps);
    const float4 o = make_float4((v.x - mean) * rstd * g.x + bb.x, (v.y - mean) * rstd * g.y + bb.y, (v.z - mean) * rstd * g.z + bb.z,
                                 (v.w - mean) * rstd * g.w + bb.w);
    if (FINAL) {
      if (row0 + r < M) *(float4*)(out + (row0 + r) * RC_D + 4 * lane) = o;
    } else {
      *(float4*)fr = o;
      uint2 h, l;
      split_trunc_bf16x2(o.x, o.y, h.x, l.x);
      split_trunc_bf16x2(o.z, o.w, h.y, l.y);
      *(uint2*)(s_hi + r * RC_LD + 4 * lane) = h;
      *(uint2*)(s_lo + r * RC_LD + 4 * lane) = l;
    }
  }
}

__global__ __launch_bounds__(512) void rowchain_x3_kernel(const RowchainParams p) {
#if __HIP_DEVICE_COMPILE__
  __shared__ __attribute__((aligned(16))) u16 s_a[2 * RC_PLANE], s_h[2 * RC_PLANE];
  float* s_f = (float*)s_h;  // fp32 [64][RC_LDF] LayerNorm staging, over the hidden chunk's planes
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int col = 32 * wave + l31;
  const int64_t row0 = (int64_t)blockIdx.x * RC_ROWS;
  const int chunks = p.H / RC_D, ks2 = p.H / 16;

  // the first weights and the residual rows travel while x is staged
  const uint4* w_cur = p.wo + (size_t)(wave * 16) * 128 + lane;
  uint4 wb[8];
  rc_load_w(wb, w_cur);
  f32x16 rz[2];  // res, later z, in the accumulator layout: [b][r] = row 32 b + (r & 3) + 8 (r >> 2) + 4 lh, column col
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * lh;
      rz[b][r] = row < p.M ? p.res[row * RC_D + col] : 0.f;
    }
  {
    constexpr int PPT = RC_ROWS * RC_D / 4 / 512;  // 16-byte fp32 pieces per thread
    float4 nx[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int pc = i * 512 + t;
      const int64_t row = row0 + pc / (RC_D / 4);
      nx[i] = row < p.M ? *(const float4*)(p.x + row * RC_D + 4 * (pc % (RC_D / 4))) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int pc = i * 512 + t, r = pc / (RC_D / 4), c = 4 * (pc % (RC_D / 4));
      uint2 h, l;
      split_trunc_bf16x2(nx[i].x, nx[i].y, h.x, l.x);
      split_trunc_bf16x2(nx[i].z, nx[i].w, h.y, l.y);
      *(uint2*)(s_a + r * RC_LD + c) = h;
      *(uint2*)(s_a + RC_PLANE + r * RC_LD + c) = l;
    }
  }
  rc_barrier();

  const int frag = l31 * RC_LD + 8 * lh;
  const u16 *aa_hi = s_a + frag, *aa_lo = s_a + RC_PLANE + frag, *ah_hi = s_h + frag, *ah_lo = s_h + RC_PLANE + frag;
  const uint4* w1_0 = p.w1 + (size_t)(wave * 16) * 128 + lane;  // chunk c: column block 8 c + wave
  const uint4* w2_0 = p.w2 + (size_t)(wave * ks2) * 128 + lane;  // chunk c: K steps 16 c .. 16 c + 15
  f32x16 acc[2], acc2[2];
  auto zero = [](f32x16 (&v)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) v[b][r] = 0.f;
  };
  auto frow = [&](int b, int r) { return 32 * b + (r & 3) + 8 * (r >> 2) + 4 * lh; };

  // y = x Wo^T + bo + res
  zero(acc);
  rc_pass(aa_hi, aa_lo, w_cur, w1_0, wb, acc);
  {
    const float bv = p.bo[col];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) s_f[frow(b, r) * RC_LDF + col] = acc[b][r] + bv + rz[b][r];
  }
  rc_barrier();  // y complete, every wave has left the planes of x
  rc_layernorm<false>(s_f, s_a, s_a + RC_PLANE, p.g1, p.b1, p.eps1, nullptr, row0, p.M, wave, lane);
  rc_barrier();
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) rz[b][r] = s_f[frow(b, r) * RC_LDF + col];

  zero(acc2);
  const bool odd = (lane & 1) != 0;
  u16* hdst = s_h + (odd ? RC_PLANE : 0) + 32 * wave + (l31 & ~1);  // the pair's two columns in the even lane's hi / the odd lane's lo plane
  for (int c = 0; c < chunks; ++c) {
    // h = relu(z W1^T + c1), columns 256 c .. 256 c + 255
    const uint4* w1c = w1_0 + (size_t)c * (8 * 16 * 128);
    const uint4* w2c = w2_0 + (size_t)c * (16 * 128);
    zero(acc);
    rc_pass(aa_hi, aa_lo, w1c, w2c, wb, acc);
    const float cv = p.c1[c * RC_D + col];
    rc_barrier();  // every wave has read z / has left the previous chunk's planes
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = fmaxf(acc[b][r] + cv, 0.f);
        const float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
        uint32_t hi, lo;
        split_trunc_bf16x2(odd ? nb : v, odd ? v : nb, hi, lo);
        *(uint32_t*)(hdst + frow(b, r) * RC_LD) = odd ? lo : hi;
      }
    rc_barrier();
    // o += h W2[:, 256 c .. 256 c + 255]^T
    rc_pass(ah_hi, ah_lo, w2c, c + 1 < chunks ? w1c + 8 * 16 * 128 : w2c, wb, acc2);
  }

  rc_barrier();  // every wave has left the last chunk's planes
  {
    const float bv = p.c2[col];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) s_f[frow(b, r) * RC_LDF + col] = acc2[b][r] + bv + rz[b][r];
  }
  rc_barrier();
  rc_layernorm<true>(s_f, nullptr, nullptr, p.g2, p.b2, p.eps2, p.out, row0, p.M, wave, lane);
#endif
}

}  // namespace

extern "C" int siu3r_rowchain_x3(const float* x, const float* res, const void* pack, float* out, int64_t M, int H, float eps1, float eps2,
                                 void* stream) {
  SIU3R_CHECK(M > 0 && cdiv64(M, RC_ROWS) <= 0x7fffffff, "rowchain_x3: bad row count M=%lld", (long long)M);
  SIU3R_CHECK(H > 0 && H % RC_D == 0, "rowchain_x3: H=%d must be a positive multiple of 256", H);
  SIU3R_CHECK(x && res && pack && out, "rowchain_x3: null pointer");
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  SIU3R_CHECK(al16(x) && al16(res) && al16(pack) && al16(out), "rowchain_x3: x, res, pack and out must be 16-byte aligned");
  // pack (ops.pack_rowchain): Wo | W1 | W2 fragments (bf16 hi / lo), then fp32 bo, g1, b1, c2, g2, b2 [256 each], c1 [H]
  const char* pk = (const char*)pack;
  const size_t wo_b = (size_t)RC_D * RC_D * 4, w1_b = (size_t)H * RC_D * 4;
  const float* vec = (const float*)(pk + wo_b + 2 * w1_b);
  RowchainParams p{x, res, (const uint4*)pk, (const uint4*)(pk + wo_b), (const uint4*)(pk + wo_b + w1_b),
                   vec, vec + RC_D, vec + 2 * RC_D, vec + 3 * RC_D, vec + 4 * RC_D, vec + 5 * RC_D, vec + 6 * RC_D, out, M, H, eps1, eps2};
  hipLaunchKernelGGL(rowchain_x3_kernel, dim3((unsigned)cdiv64(M, RC_ROWS)), dim3(512), 0, (hipStream_t)stream, p);
  SIU3R_LAUNCH_CHECK("siu3r_rowchain_x3");
  return 0;
}
