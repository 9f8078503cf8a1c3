/*
 * siu3r_hip.h -- C ABI of libsiu3r_hip.so, the MI355X (gfx950) hot path of SIU3R inference.
 *
 * Conventions:
 *   - every entry point returns 0 on success, non-zero on error; siu3r_last_error() returns a
 *     thread-local message.  The Python wrappers raise RuntimeError, mirroring the reference's
 *     TORCH_CHECK behaviour (reference: src/models/croco/curope/curope.cpp:54-59, kernels.cu:91-94).
 *   - all pointers are raw DEVICE pointers unless stated; no entry point allocates, synchronises
 *     or owns memory; kernels are enqueued on `stream` (a hipStream_t passed as void*).
 *   - dtype codes: SIU3R_BF16 = 0, SIU3R_F32 = 1 everywhere; siu3r_rope2d (seam 1) also takes SIU3R_F16 = 2 and SIU3R_F64 = 3,
 *     the types the reference's kernel dispatches (kernels.cu:101).
 *   - activations are channel-last ("NHWC" / token-major) everywhere.
 *
 * Each group cites the reference interface it replaces.
 */
#ifndef SIU3R_HIP_H
#define SIU3R_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SIU3R_BF16 0
#define SIU3R_F32 1
#define SIU3R_F16 2
#define SIU3R_F64 3

const char* siu3r_last_error(void);
#define SIU3R_ABI_VERSION 13 /* 13: siu3r_panoptic_stage1 takes the overlap threshold as a double (the reference compares the float32 area ratio with the double 0.8: a ratio that rounds to fp32(0.8) is accepted); 12: siu3r_gemm_plan_t.skinny_path (which code multiplies the remainder rows); 11: siu3r_attention_plan (what siu3r_attention launches for a parameter block); 10: siu3r_stem7x7_x3 (the Gaussian heads' stem as one dedicated kernel), siu3r_proj_rows_x3 (the heads' last 1 x 1 convolutions as row streams); 9: siu3r_raster_project_c2w + siu3r_raster_cam.k2_near / k2_far (the reference renderer's own pose tensors, consumed on the device), siu3r_raster_tune (replaces the SIU3R_FEAT_FORM / SIU3R_FEAT_NP environment switches; the shared-batch matrix-core composite is gone: no workspace = 32-channel kernel); 8: LPIPS (siu3r_maxpool2x2s2, siu3r_lpips_layer); 7: device-side poses for the gsplat seam (siu3r_raster_project_dp, siu3r_sh_eval_dp, siu3r_blend_background_dp), precomputed K2 colours (sh_degree < 0), all-channel list composite; 6: pre-split bf16x3 activations (siu3r_gemm_params.c_x3 / a_x3, siu3r_gemm_plan_t.a_x3_ok / c_x3_ok), siu3r_attn_params.kv_bxor / kv_x3, siu3r_gemm_params.c_x3_col0; 5: siu3r_raster_sort takes stage 1's counters (culled Gaussians leave the sort), NaN-poisoned views on entry overflow, siu3r_gemm_tune key 4; 4: siu3r_gemm_plan, split-K workspace capacities + self-resetting tickets, tile_cfg; 3: view-batched sort-free rasterizer */
int siu3r_abi_version(void);

/* ---- seam 1: curope.rope_2d(tokens, positions, base, fwd)
 * reference: src/models/croco/curope/curope.cpp:49-65 (dispatch), kernels.cu:17-108 (kernel).
 * tokens [B,N,H,D] in place (stride_d == 1), positions int64 [B,N,2] contiguous, D % 4 == 0.    */
int siu3r_rope2d(void* tokens, int dtype, int B, int N, int H, int D, int64_t stride_b,
                 int64_t stride_n, int64_t stride_h, const int64_t* positions, float base, float fwd,
                 void* stream);

/* ---- GEMM / implicit-GEMM convolution on MFMA (bf16 operands, fp32 accumulate).
 * Replaces every nn.Linear / nn.Conv2d / nn.ConvTranspose2d(k==stride) on the path
 * (reference: croco/blocks.py:58-79,94-112; heads/dpt_block.py; vit_adapter.py; video_seg_decoder.py).
 * C[M,N] = epilogue(A[M,K] * W[N,K]^T).  W is pre-packed bf16 [N, Kpad] (Kpad % 64 == 0, zero padded);
 * w_lo (may be NULL) holds the bf16 residual of the fp32 weight and enables the 3-pass
 * "bf16x3" mode (A must then be fp32): C = Ahi*Whi + Ahi*Wlo + Alo*Whi, ~fp32 accuracy.
 * Dense A: the elements A[m, k .. kpad) behind a row (inside the operand: the row stride's slack or the next row) MAY be fetched and
 * multiplied by the zero padding of W, so they must be finite; nothing is read beyond element (m-1)*lda + k of a batch item. */
typedef struct {
  const void* a;          /* activations */
  const void* w_hi;       /* bf16 [N,Kpad] */
  const void* w_lo;       /* bf16 [N,Kpad] or NULL */
  void* c;                /* output */
  const float* bias;      /* [N] (or [Cout] for out_mode 1) or NULL */
  const void* residual;   /* added after activation, same indexing as c, or NULL */
  int32_t m, n, k, kpad;
  int64_t lda, ldc, ldr;  /* row strides in elements (dense A / C / residual) */
  int32_t a_dtype, c_dtype, r_dtype;
  int32_t act;            /* 0 none, 1 exact-erf GELU, 2 ReLU */
  int32_t relu_in;        /* apply ReLU to A while loading */
  /* batching: blockIdx.z selects the batch; strides in elements */
  int32_t batch;
  int64_t sa, sw, sc, sr;
  /* A addressing: 0 dense rows; 1 NHWC conv gather; 2 NCHW fp32 16x16 patchify (patch-embed) */
  int32_t a_mode;
  int32_t ih, iw, cin, kh, kw, stride, pad, oh, ow; /* conv geometry (a_mode 1,2) */
  /* output addressing: 0 row-major; 1 conv-transpose (kernel==stride) pixel shuffle:
     n = (ky*up+kx)*cout + co, row m=(b,iy,ix) -> out[b, iy*up+ky, ix*up+kx, co] */
  int32_t out_mode, up, cout;
  /* fused epilogue extra: bilinear x2 (align_corners=True) upsample-add of a low-res NHWC map
     (GS head: feat_up(path_1) + ReLU(conv7x7(img)), reference dpt_gs_head.py:160-162) */
  const void* up_src;     /* [B, oh/2, ow/2, n] or NULL */
  int32_t up_dtype;
  /* fused RoPE2D epilogue (reference croco/blocks.py:101-103 + curope kernels.cu:17-82) for the QKV / projq /
     projk GEMMs: output columns [0, rope_ncols) are heads of dim 64 laid out [u_Y v_Y u_X v_X]; row (z, m) is
     the token with position rope_pos[(z*m_rows + m)*2 + {y,x}]; tables are fp32 [max_pos, 16]. NULL = off. */
  const float* rope_cos;
  const float* rope_sin;
  const int64_t* rope_pos;
  int32_t rope_ncols;
  int32_t map_gx, map_rm, map_rn; /* filled by the launcher (XCD-aware tile map); callers leave them 0 */
  uint64_t* trace;                /* tuning aid, normally NULL: 8 shader-clock stamps per workgroup (tools/gemm_trace.py) */
  const void* w_x3;               /* bf16x3 on the LDS-DMA path: both planes interleaved per 32-deep K tile, bf16 [N, Kpad/32, 2, 32]
                                     (hi 32 | lo 32); NULL = use w_hi / w_lo with the register-staged kernel */
  /* two-level batching (bmod > 0): blockIdx.z = zo * bmod + zi; element offsets A: zo*sa + zi*sa_i, C: zo*sc + zi*sc_i, residual:
     zo*sr + zi*sr_i; the weight set is zi (offset zi*sw); bias / ln_c1 / ln_c2 advance by zi*sbias floats.  This is how the two
     decoder sides (dec_blocks / dec_blocks2, reference backbone_croco.py:231-255) run as ONE launch: zi = side, zo = batch item,
     and a side's cross-attention memory is the OTHER view (a negative sa_i).  bmod == 0: single level (z*sa, z*sw, z*sc, z*sr). */
  int32_t bmod;
  int64_t sa_i, sc_i, sr_i, sbias;
  /* LayerNorm folded into this GEMM (reference croco/blocks.py:127-130,186-191: x + f(LN(x))): A holds the UN-normalised rows, the
     packed weight is W diag(gamma), and the epilogue computes rstd_m * (acc - mean_m * ln_c1[n]) + ln_c2[n] with
     ln_c1[n] = sum_k W'[n,k], ln_c2[n] = sum_k beta_k W[n,k] + b[n] (bias must be NULL).  mean / rstd of row m come from ln_stats:
     ln_tiles (mean, M2) partials of 64 columns each (the last one of K - 64*(ln_tiles-1)), written by the GEMM that produced A
     (stats_out below), row (zo, zi, m) at float2 index ((zo*ln_sz + zi*ln_sz_i + m*ln_ldm) * ln_tiles). */
  const float* ln_stats;
  const float* ln_c1;
  const float* ln_c2;
  int32_t ln_tiles;
  float ln_eps;
  int64_t ln_ldm, ln_sz, ln_sz_i;
  /* row statistics of THIS GEMM's output (out_mode 0, after bias / activation / residual): per 64-column tile the mean and the
     centred sum of squares (Welford partials; merged by the consumer), float2 index ((zo*st_sz + zi*st_sz_i + m*st_ldm) * tiles_n + tile_n) */
  float* stats_out;
  int64_t st_ldm, st_sz, st_sz_i;
  void* c_aux;                    /* optional bf16 copy of the output (same indexing as c): the next GEMM's A operand in bf16 mode */
  /* split-K over workgroups: blockIdx.y = K slice; every slice writes its fp32 partial tile to sk_ws [tiles, splitk, BM * BN] and draws
     a ticket from sk_cnt [tiles] (int32, ZERO before the first launch that uses them); the last arriver of a tile sums the slabs in
     slice order (deterministic), runs the epilogue and resets the ticket, so one zero-initialised counter array serves any number
     of launches ON ONE STREAM.  For launches with few tiles and a long K (at batch 1 most of the decoder / head / Mask2Former GEMMs).
     splitk: 0 = the launcher decides (siu3r_gemm_plan; 1 when no workspace is attached), 1 = never, > 1 = this many slices (the
     workspace must hold siu3r_gemm_plan's ws_floats / counters for it).  sk_ws_floats / sk_cnt_n: capacities of the workspace. */
  int32_t splitk;
  float* sk_ws;
  int32_t* sk_cnt;
  int64_t sk_ws_floats;
  int32_t sk_cnt_n;
  int32_t tile_cfg;               /* 0 = the launcher decides; SIU3R_TILE_* forces a kernel family / tile (tools, tests) */
  int32_t m_main;                 /* internal (launcher): rows covered by the tiled kernel when a skinny launch multiplies the last <= 32 rows */
  int32_t sk_gx;                  /* internal (launcher): > 0 = the ping-pong launch carries the remainder rows itself, as workgroups blockIdx.x >= sk_gx */
  /* Pre-split bf16x3 activations.  A bf16x3 product multiplies hi = the upper 16 bits of every fp32 activation and lo = bf16(a - hi);
     the ping-pong kernels normally derive both inside their K loop, which costs 12-18 % of a launch.  c_x3 != NULL: the epilogue ALSO
     writes the (fp32, post-activation, post-residual) output as those two planes, interleaved per 32 columns like w_x3 -- row m at the
     byte offset of row m of c, then [n / 32][hi 32 | lo 32] bf16: a buffer of the size and strides of the fp32 output; c may then be
     NULL (planes only).  a_x3 != 0: `a` points at such planes (dense A only, k % 64 == 0, lda and the batch strides multiples of 32):
     same products in the same order as with the fp32 operand, hence bit-identical results.  Both need a ping-pong plan and the common
     output form (siu3r_gemm_plan_t.a_x3_ok / c_x3_ok say whether the plan of THIS block can consume / emit planes; siu3r_gemm fails
     loudly otherwise). */
  void* c_x3;
  int32_t a_x3;
  int32_t c_x3_col0;              /* planes are written for output columns >= c_x3_col0 only (a multiple of 64; 0 = all).  With c_x3 == c the
                                     buffer is MIXED: fp32 in columns [0, c_x3_col0), planes behind them (the q | k | v projection: q stays
                                     fp32, k and v are pre-split for the attention kernel) */
} siu3r_gemm_params;
#define SIU3R_TILE_AUTO 0
#define SIU3R_TILE_128x64 -1   /* the 128 x 64 LDS-DMA / register-staged kernels (gemm_dma.hip, gemm.hip) */
#define SIU3R_TILE_PP_256x256 1 /* 8-wave ping-pong kernels (gemm_pp.hip) */
#define SIU3R_TILE_PP_256x128 2
#define SIU3R_TILE_PP_128x128 3
int siu3r_gemm(const siu3r_gemm_params* p, void* stream);
/* What siu3r_gemm will launch for these parameters (same decision function): tile family, tile, split-K slices, whether the last
 * rows go to the skinny kernel, the split-K workspace it needs (fp32 elements / int32 counters) and the kernel's name as rocprofv3
 * prints it.  Callers that attach a workspace of at least this size get the split; smaller workspaces reduce splitk.
 * skinny_path says which code multiplies the skinny_rows remainder rows: 0 = there are none, 1 = extra workgroups of the tile launch
 * itself (kernel), 2 = the MFMA skinny kernel (siu3r_gemm_pp::gemm_skinny_kernel), 3 = the matrix-vector kernel
 * (siu3r_gemm_pp::gemm_skinny_gemv_kernel); 2 and 3 are a second launch, or the only one when skinny_rows == m. */
typedef struct {
  int32_t tile_cfg, bm, bn, splitk, skinny_rows, counters;
  int64_t ws_floats;
  char kernel[160];
  int32_t a_x3_ok, c_x3_ok; /* this plan can read A as pre-split planes (a_x3) / write the output as planes (c_x3) */
  int32_t skinny_path;      /* 0 none, 1 carried by the tile launch, 2 MFMA skinny kernel, 3 matrix-vector kernel */
} siu3r_gemm_plan_t;
int siu3r_gemm_plan(const siu3r_gemm_params* p, siu3r_gemm_plan_t* out);
/* tuning aid (tools/, tests): key 0 = process-wide default of siu3r_gemm_params.tile_cfg (SIU3R_TILE_*; also env SIU3R_GEMM_PP), key 1 =
 * 1 disables the skinny remainder-row launch, key 2 = 1 disables split-K, key 3 = 1 ignores the table of measured tile choices
 * (csrc/gemm_tuned.h; also env SIU3R_GEMM_NO_TUNED) so that every problem is priced by the cost model, key 4 = 1 sends the remainder
 * rows to the skinny launch whenever it is applicable (tests).  Not for concurrent use. */
int siu3r_gemm_tune(int key, int value);

/* ---- LayerNorm over the last dim (fp32 in, act-dtype out); reference: nn.LayerNorm call sites
 * croco/blocks.py:127-191 (eps 1e-6), video_seg_decoder.py:945-1018 (eps 1e-5). */
int siu3r_layernorm(const float* x, void* y, int y_dtype, const float* gamma, const float* beta,
                    int64_t rows, int C, int64_t ldx, int64_t ldy, float eps, void* stream);
/* same, plus a second bf16 copy y2 of the result (row stride ldy2): the fp32 output remains the residual stream, the bf16 one is
 * the next GEMM's A operand */
int siu3r_layernorm2(const float* x, void* y, int y_dtype, void* y2_bf16, const float* gamma, const float* beta, int64_t rows, int C,
                     int64_t ldx, int64_t ldy, int64_t ldy2, float eps, void* stream);

/* ---- fused attention (flash style, online softmax), head_dim 64 or 32.
 * Replaces Attention/CrossAttention (croco/blocks.py:94-112,149-169, incl. RoPE2D on q,k) and
 * the Mask2Former decoder attentions (video_seg_decoder.py:782-912, nn.MultiheadAttention 946-983).
 * q,k,v: element strides (batch, token, head); head_dim contiguous.  out [B,Nq,H*D] contiguous.
 * rope_cos/sin: fp32 [max_pos, D/4] tables or NULL; qpos/kpos int64 [B,N,2] (y,x).
 * mask: uint8 [B,Nq,mask_ld] (1 = blocked; row stride mask_ld >= Nk, multiple of 64), shared by all heads, or NULL. split3 = bf16x3 mode (fp32 io). */
typedef struct {
  const void *q, *k, *v;
  void* out;
  int32_t dtype;          /* dtype of q,k,v,out */
  int32_t B, H, Nq, Nk, D;
  int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh;
  float scale;
  const float *rope_cos, *rope_sin;
  int32_t rope_max_pos;
  const int64_t *qpos, *kpos;
  const uint8_t* mask;
  int32_t split3;
  int64_t mask_ld;        /* bytes per mask row (>= Nk, multiple of 64; padding bytes are ignored) */
  float* ws;            /* split-KV workspace, fp32 [B, H, splits, ceil(Nq/128)*128, D + 4] (partial O, running max, partial sum, 2 pad);
                           NULL = no split */
  int32_t splits;       /* > 1: the keys are cut into `splits` ranges of whole 64-key tiles, one workgroup per (query tile, range),
                           combined by a second kernel.  Fast paths only (bf16, or fp32 with split3; no RoPE-on-load): few query tiles
                           against many keys (Mask2Former's 100 queries x 512..8192 keys) */
  int32_t kv_bxor;      /* batch item b reads the K / V of batch item b ^ kv_bxor (0: its own).  The two decoder sides of a pair are batch items
                           2b and 2b + 1 and a side's cross-attention memory is projected from the OTHER side's rows: with the K / V
                           projection merged into the launch that also makes q / k / v of the row's own side, the memory of side g lies in
                           the row block of side 1 - g (kv_bxor = 1).  B must be a multiple of kv_bxor + 1 (power of two). */
  int32_t kv_x3;        /* bf16x3 (fp32 tensors, split3): k and v point at PRE-SPLIT planes -- per token and head the 64 dims as two 128-byte
                           segments [hi 32 | lo 32] bf16, as a projection GEMM writes them with c_x3 / c_x3_col0 -- same strides as the
                           fp32 tensors.  Served by the pipelined kernel only (siu3r_attention_kv_x3_ok); anything else is an error. */
  int32_t out_x3;       /* bf16x3: `out` is written as PRE-SPLIT planes instead of fp32 values -- per query and 32 columns one 128-byte line
                           [hi 32 | lo 32] bf16 (hi = the upper 16 bits, lo = bf16(value - hi)), the A operand a ping-pong GEMM reads with
                           siu3r_gemm_params.a_x3 -- same size and strides as the fp32 output.  Every store of the pipelined kernel (query
                           body, key-half merge, side-path query) has this form; served by that kernel only, `out` 128-byte aligned
                           (siu3r_attention_out_x3_ok); anything else is refused before a launch.  (The field takes the struct's tail
                           padding: a zero-initialised block of an older caller means fp32.) */
} siu3r_attn_params;
int siu3r_attention(const siu3r_attn_params* p, void* stream);
/* 1 if siu3r_attention would accept these parameters with out_x3 = 1 (the pipelined kernel's conditions: head_dim 64, no mask / RoPE-on-load /
 * key split, >= 64 keys, fp32 + split3; `out` 128-byte aligned), else 0 */
int siu3r_attention_out_x3_ok(const siu3r_attn_params* p);
/* 1 if siu3r_attention would accept these parameters with kv_x3 = 1 (head_dim 64, no mask / RoPE-on-load / key split, >= 64 keys,
 * fp32 + split3, segment-aligned K / V rows), else 0 */
int siu3r_attention_kv_x3_ok(const siu3r_attn_params* p);
/* What siu3r_attention will launch for these parameters (same validation, same decision function; launches nothing): the kernel's name
 * as rocprofv3 prints it -- "siu3r_attn_pipe::attn_pipe_kernel<X3, KVP>" (8-wave pipelined kernel), "attn_fast_kernel<D, MASK, SPLITKV,
 * X3, KH>" (fast kernels) or "attn_kernel<D, IN_F32, SPLIT, MASK, QKX>" (register-staged kernels: RoPE on load, fp32 tensors without
 * split3, SIU3R_ATTN_NO_FAST; QKX = 1 with RoPE on load and bf16 operands: the rotated q and k are split for the score product) --, the queries one workgroup covers, the key ranges launched per query tile (splits, else 1), whether
 * attn_combine_kernel<D> follows, whether wave pairs share 32 queries and take one 32-key half of every tile each, and whether the
 * pipelined kernel carries query Nq - 1 (Nq = 128 n + 1) as the side path of each problem's last workgroup. */
typedef struct {
  char kernel[160];
  int32_t queries_per_wg, key_ranges, combine, key_halves, side_path;
} siu3r_attn_plan_t;
int siu3r_attention_plan(const siu3r_attn_params* p, siu3r_attn_plan_t* out);

/* ---- element-wise / gather kernels (see DESIGN.md for the HBM roofline of each) ---------- */
/* Contract shared by the entry points of this section, siu3r_layernorm / siu3r_layernorm2 / siu3r_rope2d above and siu3r_split_bf16 below:
 *  - EMPTY INPUT: a call whose element count is 0 (N = 0, rows = 0, n = 0, Q = 0, B = 0, ...) returns 0 without launching anything, after the
 *    shape arguments have been validated; the data pointers are not looked at (an empty tensor's pointer may be null).
 *  - ALIGNMENT: the kernels move four channels per lane.  The base pointers of the tensors they read or write that way -- x / y / addend of
 *    resize, affine_add, the max-pools, dwconv3x3_gelu and groupnorm, a / b / y of add, value / out of msdeform_sample, y / y2 of the
 *    LayerNorms -- must be 16-byte aligned for fp32 and 8-byte aligned for bf16; the fp32 x / gamma / beta of the LayerNorms, w9c of
 *    dwconv3x3_gelu and out of pack_image_nhwc (one pixel per store) 16-byte aligned.  A misaligned pointer is refused (non-zero return, siu3r_last_error) before anything is launched.
 *    C % 4 == 0 and the *_batch_stride % 4 == 0 / ld* % 4 == 0 rules keep every row aligned behind an aligned base.  Per-channel vectors read
 *    one value at a time (ch_scale, ch_shift, bias, GroupNorm's gamma / beta) and the operands of pts3d_exp, m2f_attn_mask and
 *    split_bf16 need only their natural alignment.  siu3r_gaussian_adapter and the offs_aw operand of siu3r_msdeform_sample take any
 *    4-byte aligned pointer and use their 16-byte loads only when the pointer allows it. */
/* y = a + b (b broadcast over rows when b_rows < rows: row r uses b[r % b_rows]) */
int siu3r_add(const float* a, const float* b, float* y, int64_t rows, int64_t b_rows, int C, void* stream);
/* image [N,3,H,W] fp32 (NCHW) -> [N,H,W,cpad] channel-last, zero padded channels: cpad = 8 (bf16 or fp32) or 4 (fp32: one 16-byte
 * pixel per gather chunk of the bf16x3 convolution) */
int siu3r_pack_image_nhwc(const float* img, void* out, int out_dtype, int N, int H, int W, int cpad, void* stream);
/* bilinear resize NHWC; align_corners as in F.interpolate; y = affine(resize(x) + addend)
 * (heads/dpt_block.py:230-235 align=1; vit_adapter.py:429-433, video_seg_decoder.py:2173-2178 align=0) */
int siu3r_resize_bilinear(const void* x, int x_dtype, void* y, int y_dtype, const void* addend, int add_dtype,
                          const float* ch_scale, const float* ch_shift, int N, int IH, int IW, int OH, int OW,
                          int C, int align_corners, void* stream);
/* the same on batch-strided inputs: x [N,IH,IW,C] / addend [N,OH,OW,C] whose batch items lie x_batch_stride / addend_batch_stride
 * elements apart (token maps that are views of a longer per-item sequence: vit_adapter.py:393-433 reads them in place) */
int siu3r_resize_bilinear_strided(const void* x, int x_dtype, void* y, int y_dtype, const void* addend, int add_dtype,
                                  const float* ch_scale, const float* ch_shift, int N, int IH, int IW, int OH, int OW,
                                  int C, int align_corners, int64_t x_batch_stride, int64_t addend_batch_stride, void* stream);
/* PLANES OUTPUT of the producers whose only reader is a bf16x3 GEMM (siu3r_resize_bilinear_planes, siu3r_dwconv3x3_gelu_planes,
 * siu3r_msdeform_sample_planes; the attention kernel has siu3r_attn_params.out_x3): the fp32 result is not stored; in its place, with the
 * size and strides of the fp32 tensor, go the pre-split planes a ping-pong GEMM reads as its A operand (siu3r_gemm_params.a_x3) -- per row
 * and 32 columns one 128-byte line [hi 32 | lo 32] bf16, hi = the upper 16 bits of the value, lo = bf16(value - hi), the split of the
 * GEMM's K loop and of its c_x3 epilogue (csrc/common.h split_trunc_bf16x2), so that the consumer multiplies the same bits.
 * REFUSED before anything is launched (non-zero return, siu3r_last_error, nothing written): a row width that is not a multiple of 32
 * (C % 32, heads * d % 32), a planes pointer that is not 128-byte aligned, and what the fp32 entry point refuses.  An empty input
 * returns 0 as above.  A caller whose shape does not qualify keeps the fp32 entry point. */
/* the plain resize (no addend, no scale / shift) of siu3r_resize_bilinear_strided, fp32 planes out */
int siu3r_resize_bilinear_planes(const void* x, int x_dtype, void* y_planes, int N, int IH, int IW, int OH, int OW, int C, int align_corners,
                                 int64_t x_batch_stride, void* stream);
/* y = x*scale[c] + shift[c] (+ addend) ; eval-mode BatchNorm folded (vit_adapter.py:436-440) */
int siu3r_affine_add(const void* x, int x_dtype, const void* addend, int add_dtype, void* y, int y_dtype,
                     const float* ch_scale, const float* ch_shift, int64_t rows, int C, void* stream);
/* rows = batch items x rows_per_batch; batch items of x / addend lie *_batch_stride elements apart; y is dense */
int siu3r_affine_add_strided(const void* x, int x_dtype, const void* addend, int add_dtype, void* y, int y_dtype,
                             const float* ch_scale, const float* ch_shift, int64_t rows, int C, int64_t rows_per_batch,
                             int64_t x_batch_stride, int64_t addend_batch_stride, void* stream);
/* 3x3 stride-2 pad-1 max pool, NHWC (vit_adapter.py:226) */
int siu3r_maxpool3x3s2(const void* x, void* y, int dtype, int N, int IH, int IW, int C, void* stream);
/* 2x2 stride-2 max pool (floor), NHWC: the pooling of the VGG16 feature stack under the evaluator's LPIPS (evaluator.py:55-57, 263) */
int siu3r_maxpool2x2s2(const void* x, void* y, int dtype, int N, int IH, int IW, int C, void* stream);
/* one feature tap of LPIPS (torchmetrics LearnedPerceptualImagePatchSimilarity("vgg"); third-party, absent from the reference tree):
 * dist[p] = sum_c w[c] * (f0[p][c] / sqrt(eps + |f0[p]|^2) - f1[p][c] / sqrt(eps + |f1[p]|^2))^2 for f0, f1 [npix, C] fp32, w [C] */
int siu3r_lpips_layer(const float* f0, const float* f1, const float* w, float* dist, int64_t npix, int C, float eps, void* stream);
/* The Gaussian heads' stem, bf16x3: out = ReLU(conv7x7(img, pad 3) + bias) + up_x2_bilinear_align_corners(up_src)
 * (reference src/models/heads/dpt_gs_head.py:71-77 input_merger = Conv2d(3, 256, 7, 1, 3) + ReLU, :158-162 feat_up(path_1) + direct_img_feat).
 * img [B, G, H, W, 4] fp32 (RGB + one zero channel); G weight sets (head g of every batch item): wfrag = MFMA B fragments of the
 * [256, 3, 7, 7] weights, [G][8][14][2][64] x 8 bf16 (siu3r_amd/ops.py pack_stem7: K ordered (ky, kx in 0..7, c in 0..3), hi = bf16(w),
 * lo = bf16(w - hi)); bias [G, 256] or NULL; up_src [B, G, H/2, W/2, 256] fp32 or NULL; out [B, G, H, W, 256]: fp32 values, or
 * (planes_out != 0) the pre-split planes a ping-pong GEMM reads as its A operand (siu3r_gemm_params.a_x3: per pixel and 32 channels one
 * 128-byte line [hi 32 | lo 32]).  H and W multiples of 16.  Same bf16x3 arithmetic as siu3r_gemm's convolution, another K order. */
int siu3r_stem7x7_x3(const float* img, const void* wfrag, const float* bias, const float* up_src, float* out, int B, int G, int H, int W,
                     int planes_out, void* stream);
/* The last 1 x 1 convolution of a DPT head as a row stream, bf16x3: out[z, m, 0..N) = x[z, m, :] W_g^T + b_g, g = z % G
 * (reference src/models/heads/dpt_block.py:384-391 gs_params head, Conv2d(256, 83, 1); :357-369 regression head, Conv2d(128, 3 + conf, 1)).
 * x [Z, M, K] fp32 with contiguous rows; wfrag = MFMA B fragments of the G weight matrices [N, K], [G][ceil(N/32)][K/16][2][64] x 8 bf16
 * (siu3r_amd/ops.py pack_proj); bias [G, 32 ceil(N/32)] zero padded, or NULL; out [Z, M, N] fp32 with row stride ldc floats and
 * out_z_stride floats between consecutive z (0 = M * ldc).
 * Instantiations: K = 256 with 65 <= N <= 96, K = 128 with N <= 32.  Same bf16x3 products as siu3r_gemm, another K order. */
int siu3r_proj_rows_x3(const float* x, const void* wfrag, const float* bias, float* out, int Z, int G, int64_t M, int K, int N, int ldc,
                       int64_t out_z_stride, void* stream);
/* The row chain that ends a Mask2Former pixel-decoder encoder layer (reference video_seg_decoder.py:945-1018) as one launch, bf16x3,
 * d_model = 256, for rows [0, M) of contiguous [M, 256] fp32 tensors:
 *   y = x Wo^T + bo + res;  z = LN(y; g1, b1, eps1);  h = relu(z W1^T + c1);  o = h W2^T + c2 + z;  out = LN(o; g2, b2, eps2)
 * with Wo [256, 256], W1 [H, 256], W2 [256, H], H a multiple of 256 (the hidden layer is produced and consumed on chip in 256-column
 * chunks).  Every product is A_hi W_hi + A_lo W_hi + A_hi W_lo with fp32 accumulation, A split as siu3r_gemm splits it (hi = the upper
 * 16 bits, lo = bf16(a - hi)), K ascending in steps of 16 and per step hi x hi, hi x lo, lo x hi, then bias, activation, residual: the
 * order of siu3r_gemm's ping-pong kernels, so that on shapes those kernels serve the result equals the five separate launches bit for
 * bit; the LayerNorms are siu3r_layernorm's (fp32, the mean first, then the centred sum of squares; the same sums at C = 256).
 * pack (siu3r_amd/ops.py pack_rowchain): the fragments of Wo, W1, W2 in siu3r_proj_rows_x3's layout, one after the other, then fp32
 * bo, g1, b1, c2, g2, b2 [256 each] and c1 [H].  No atomics: two launches on the same inputs give the same bits.
 * REFUSED before anything is launched (non-zero return, siu3r_last_error, nothing written): a null pointer, M <= 0 (an empty M is
 * refused as siu3r_proj_rows_x3 refuses it: the caller skips the call), H that is not a positive multiple of 256, a base pointer that
 * is not 16-byte aligned.  out may NOT alias x or res: a workgroup's rows are read and written at different times. */
int siu3r_rowchain_x3(const float* x, const float* res, const void* pack, float* out, int64_t M, int H, float eps1, float eps2, void* stream);
/* depth-wise 3x3 + bias + GELU over the 3 token scales of the adapter ConvFFN (vit_adapter.py:16-59) */
int siu3r_dwconv3x3_gelu(const void* x, void* y, int dtype, const float* w9c, const float* bias, int B, int H,
                         int W, int C, void* stream);
/* the same with fp32 x and the result as pre-split planes (PLANES OUTPUT above: C % 32 == 0) */
int siu3r_dwconv3x3_gelu_planes(const float* x, void* y_planes, const float* w9c, const float* bias, int B, int H, int W, int C, void* stream);
/* multi-scale deformable attention sampling core (vit_adapter/blocks.py:217-267):
 * value [B,S,heads,d]; offs_aw fp32 [B,Q,heads*L*P*3] = per row [offsets (h,L,P,2) | logits (h,L,P)];
 * ref fp32 [Q,L,2]; shapes int32 [L,2] (h,w) host pointer; out [B,Q,heads*d]. */
int siu3r_msdeform_sample(const void* value, int v_dtype, const float* offs_aw, const float* ref,
                          const int32_t* shapes_host, void* out, int out_dtype, int B, int S, int Q, int heads,
                          int d, int L, int P, void* stream);
/* the same with the result as pre-split planes (PLANES OUTPUT above: heads * d % 32 == 0).  Only the kernels specialised for the level
 * count write planes: L = 1, 3 or 4 with P = 4 and a 16-byte aligned offs_aw; anything else is refused. */
int siu3r_msdeform_sample_planes(const void* value, int v_dtype, const float* offs_aw, const float* ref, const int32_t* shapes_host,
                                 void* out_planes, int B, int S, int Q, int heads, int d, int L, int P, void* stream);
/* GroupNorm(32) on NHWC (video_seg_decoder.py:2002-2050): two kernels, stats then apply
 * y = relu?(gn(x)) + addend? ; stats is a [N,groups,2] fp32 workspace */
int siu3r_groupnorm(const void* x, int x_dtype, void* y, int y_dtype, const float* gamma, const float* beta,
                    float* stats_ws, const void* addend, int add_dtype, int relu, int N, int HW, int C,
                    int groups, float eps, void* stream);
/* pts3d = xyz/|xyz| * expm1(|xyz|)  (heads/postprocess.py:45-61), in place on [n,3] fp32 */
int siu3r_pts3d_exp(float* xyz, int64_t n, void* stream);
/* UnifiedGaussianAdapter.forward (gaussian_adapter.py:81-110): raw [n,83] -> fields (all fp32) */
int siu3r_gaussian_adapter(const void* raw, int raw_dtype, float* opacities, float* scales, float* rotations,
                           float* harmonics, float* covariances, int64_t n, void* stream);
/* Mask2Former attention mask (video_seg_decoder.py:1461-1478 + 1306-1308): mask logits
 * [B,T,IH,IW,Q] (channel-last) -> uint8 [B,Q,out_ld] (first T*OH*OW bytes of each row), 1 = blocked; rows fully
 * blocked are cleared.  row_counts_ws: B*Q int32 of scratch (zeroed by the call; holds a "row has an open key" flag). */
int siu3r_m2f_attn_mask(const float* mask_logits, uint8_t* out, int32_t* row_counts_ws, int B, int T, int IH,
                        int IW, int OH, int OW, int Q, int64_t out_ld, void* stream);

/* ---- Gaussian splat rasterizer (tile-binned, all views of a call in every launch).  Replaces the reference's two
 * un-vendored CUDA dependencies at their call sites: GaussianRasterizer(settings)(means3D, ..., cov3D_precomp, ...) ->
 * (image, radii, depth, opacity, n_touched) (reference src/models/cuda_splatting.py:90-118; mode 0) and
 * gsplat.rasterization(means, covars, opacities, colors[N,C], viewmats, Ks, width, height, near_plane, far_plane) ->
 * (colors, alphas, meta) (reference src/models/gaussian_renderer.py:92-106; mode 1).  The reference loops over the views in
 * Python (cuda_splatting.py:82-121); here V cameras go in as one HOST array (copied to `cams_dev` on the stream) and
 * blockIdx.y is the view.  All constants of the published algorithms are explicit parameters.
 * Stages: project -> sort (one stable depth radix sort per view) -> bin (depth-ordered coarse bins of cb x cb tiles) ->
 * composite_rgb (mode 0; walks the bins, no per-tile lists) | tile_lists + composite_feat (mode 1). */
typedef struct {
  int32_t mode;        /* 0 = K2 (3DGS family), 1 = K3 (gsplat family) */
  int32_t width, height;
  float w2c[16];       /* world->camera, row-major (column-vector convention) */
  float proj[16];      /* K2: full projection P = Proj * W2C, row-major */
  float tanfovx, tanfovy;
  float campos[3];
  float bg[3];
  int32_t sh_degree;   /* K2: 0..4; -1 = `colors` are precomputed [G,3] colours, blended as given (no SH, no +0.5, no clamp) */
  int32_t sh_band4;    /* K2: evaluate SH coefficients 16..24 (open question of the fork; default 0) */
  float k2_znear_cull; /* 0.2 */
  float fx, fy, cx, cy; /* K3: pixel-unit intrinsics */
  float near_plane, far_plane; /* K3; near_plane must be > 0 (depth keys are the float bit patterns) */
  float eps2d;         /* 0.3 */
  float radius_clip;
  float extent_sigma;  /* 3.33 */
  int32_t opacity_aware_extent;
  float alpha_min;     /* 1/255 */
  float alpha_max;     /* 0.99 (K2) / 0.999 (K3) */
  float t_min;         /* 1e-4 */
  float dilation;      /* K2 low-pass 0.3 */
  int32_t nt_post_blend; /* K2 n_touched: count a pixel when the transmittance AFTER blending the Gaussian is > 0.5
                            (1, the MonoGS fork's `test_T > 0.5f`) or the one before it (0) */
  float k2_near, k2_far; /* K2, siu3r_raster_project_c2w only: the planes of the [0, 1]-depth projection matrix the device derives
                            (cuda_splatting.py:16-43); ignored when `proj` is given by the host */
} siu3r_raster_cam;
/* frame geometry / workspace sizes: out8 = {gw, gh, T = tiles, cb = coarse-bin edge in tiles, NB = coarse bins,
 * nchunks_sort (columns of rs_hist), nchunks_bin (columns of bin_hist), sizeof(siu3r_raster_cam)} */
int siu3r_raster_geometry(int width, int height, int64_t G, int32_t* out8);
/* stage 1: project G Gaussians (means [G,3]; cov: cov_stride 6 = upper-triangular (xx,xy,xz,yy,yz,zz), 9 = row-major 3x3;
 * opacities [G]; colors: mode 0 SH coefficients, sh_planar 0 = [G,channels,3] (the layout of cuda_splatting.py:65), 1 = [G,3,25]
 * (Gaussians.harmonics as stored), mode 1 unused; all shared by the V views) for every view.  cams_host: V structs in HOST memory,
 * copied to cams_dev (device, V * sizeof(siu3r_raster_cam) bytes) on the stream.  Outputs, all [V, G, ...]: rec fp32 [.,12] = {mean2d x, y,
 * depth, 0 | conic a, b, c, opacity | r, g, b, 0} (16-byte aligned), radii [.,2] i32, rect [.,4] i32 (tile rect [min,max)),
 * tiles_touched i32, keys u32 (depth bits; 0xffffffff = culled; a Gaussian whose mean or covariance is not finite is culled in every
 * view).  stats: u64 [V,4] = {visible Gaussians, tile pairs D, coarse
 * entries E (stage 3), flags: bit 0 entries overflowed cap_e, bit 1 tile lists overflowed cap_d}; zeroed here. */
int siu3r_raster_project(const siu3r_raster_cam* cams_host, int V, void* cams_dev, int64_t G, const float* means, const float* cov,
                         int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, float* rec,
                         int32_t* radii, int32_t* rect, int32_t* tiles_touched, uint32_t* keys, uint64_t* stats, void* stream);
/* the same with the POSE in device memory, gsplat family (mode 1) only -- what gsplat.rasterization receives (reference
 * src/models/gaussian_renderer.py:92-106, viewer.py:319-335): viewmats_dev [V,4,4] world->camera and Ks_dev [V,3,3] pixel-unit
 * intrinsics, row-major fp32 device tensors; they overwrite w2c / fx / fy / cx / cy of the uploaded camera blocks on the stream, so that
 * the host never reads a pose back (no synchronisation).  cams_host carries everything else (frame size, planes, thresholds). */
int siu3r_raster_project_dp(const siu3r_raster_cam* cams_host, int V, void* cams_dev, const float* viewmats_dev, const float* Ks_dev, int64_t G,
                            const float* means, const float* cov, int cov_stride, const float* opacities, const float* colors, int channels,
                            int sh_planar, float* rec, int32_t* radii, int32_t* rect, int32_t* tiles_touched, uint32_t* keys, uint64_t* stats,
                            void* stream);
/* the same with the pose AS THE REFERENCE'S RENDERER HOLDS IT (SplattingCUDA.forward, src/models/gaussian_renderer.py:29-74; render_cuda,
 * cuda_splatting.py:46-121), both families: c2w_dev [V,4,4] camera-to-world extrinsics and Kn_dev [V,3,3] NORMALISED intrinsics, row-major
 * fp32 device tensors.  A one-thread-per-view kernel on the stream derives w2c = inverse(c2w with its translation * t_scale), campos and,
 * mode 0: fov from the K^-1 edge rays (utils/projection.py:247-261), tanfovx / tanfovy, proj = Proj(k2_near, k2_far, fov) * w2c; mode 1:
 * fx, fy, cx, cy = K * (width, height) -- in fp64, rounded once -- and overwrites those fields of the uploaded blocks: no pose value is
 * read on the host (the reference's .inverse() / get_fov run on its device too).  A singular c2w gives a NaN pose (nothing passes the depth test). */
int siu3r_raster_project_c2w(const siu3r_raster_cam* cams_host, int V, void* cams_dev, const float* c2w_dev, const float* Kn_dev, float t_scale,
                             int64_t G, const float* means, const float* cov, int cov_stride, const float* opacities, const float* colors,
                             int channels, int sh_planar, float* rec, int32_t* radii, int32_t* rect, int32_t* tiles_touched, uint32_t* keys,
                             uint64_t* stats, void* stream);
/* ---- anti-aliased projection, 3DGS family (the 2-D filter of Mip-Splatting, Yu et al. 2024: upstream 3DGS's
 * GaussianRasterizationSettings.antialiasing; additions, ABI version unchanged).  siu3r_raster_project / siu3r_raster_project_c2w with one
 * more argument, comp, in front of the stream.  Per (view, Gaussian), with c00', c01, c11' the 2-D covariance entries BEFORE the camera's
 * dilation B is added to the diagonal (the values themselves, not c00 - B), det1 the determinant of the dilated covariance (what the conic
 * is divided by) and det0 = c00' c11' - c01^2 in Kahan's form (the rounding error of c01 * c01 recovered by one fma: a thin diagonal splat
 * cancels badly in the naive form):
 *   comp = sqrtf(fmaxf(2.5e-5f, det0 / det1)),   rec[.., 7] = opacity * comp   (where the rect is non-empty; elsewhere rec[.., 7] = opacity)
 * so that the dilated footprint integrates to what the undilated one does (comp sqrt(det1) = sqrt(det0)) instead of growing brighter; the
 * floor is upstream's.  comp [V, G] fp32 (optional, NULL = not wanted) receives the factor where the rect is non-empty and 0 elsewhere.
 * The other eleven record slots, radii, rect, tiles_touched, keys and stats are the bits of the classic call; sort, bin, the composites,
 * their backwards and siu3r_raster_contrib read the record's opacity and follow without change.  Mode 0 only: a mode-1 view array is refused. */
int siu3r_raster_project_aa(const siu3r_raster_cam* cams_host, int V, void* cams_dev, int64_t G, const float* means, const float* cov,
                            int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, float* rec,
                            int32_t* radii, int32_t* rect, int32_t* tiles_touched, uint32_t* keys, uint64_t* stats, float* comp, void* stream);
int siu3r_raster_project_c2w_aa(const siu3r_raster_cam* cams_host, int V, void* cams_dev, const float* c2w_dev, const float* Kn_dev, float t_scale,
                                int64_t G, const float* means, const float* cov, int cov_stride, const float* opacities, const float* colors,
                                int channels, int sh_planar, float* rec, int32_t* radii, int32_t* rect, int32_t* tiles_touched, uint32_t* keys,
                                uint64_t* stats, float* comp, void* stream);
/* stage 2: per view, stable LSD radix sort (4 x 8 bits) of keys_a [V,G] with the Gaussian index as payload; keys_b / ids_a / ids_b
 * [V,G] ping-pong buffers; rs_hist i32 [V,256,nchunks_sort], rs_tot i32 [V,256]; stats: stage 1's counters (device).  Culled Gaussians
 * (key 0xffffffff) leave the sort in its first pass: the result is the (depth, id)-ordered list of the n = stats[v][0] VISIBLE Gaussians in
 * keys_a / ids_a [v][0, n); what lies behind is unspecified (stage 3 reads n from stats as well). */
int siu3r_raster_sort(int V, int64_t G, uint32_t* keys_a, uint32_t* keys_b, int32_t* ids_a, int32_t* ids_b, int32_t* rs_hist,
                      int32_t* rs_tot, const uint64_t* stats, void* stream);
/* stage 3: depth-ordered coarse bins.  bin_hist i32 [V,NB,nchunks_bin], bin_tot i32 [V,NB], bin_start i32 [V,NB+1] (out),
 * entries: 8-byte records [V,cap_e] (Gaussian id, rect clipped to the bin).  Entries beyond cap_e are dropped and flagged in
 * stats (the true count is stats[v][2]): size by a bound, enqueue the whole frame, check once afterwards. */
int siu3r_raster_bin(const siu3r_raster_cam* cams_host, int V, int64_t G, const uint32_t* keys, const int32_t* ids, const int32_t* rect,
                     int32_t* bin_hist, int32_t* bin_tot, int32_t* bin_start, void* entries, int64_t cap_e, uint64_t* stats, void* stream);
/* stage 4 (mode 0): image [V,3,H,W], depth [V,H,W], accumulated opacity [V,H,W], n_touched [V,G] i32 (NULL = not wanted).
 * A view whose entries overflowed cap_e (bin_start[v][NB] > cap_e) gets NaN in every output pixel: never a subtly wrong image, so the
 * caller may read stats late (asynchronously) and repeat the call with a larger cap_e. */
int siu3r_raster_composite_rgb(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                               const void* entries, int64_t cap_e, const float* rec, float* image, float* out_depth, float* out_alpha,
                               int32_t* n_touched, void* stream);
/* per-tile Gaussian lists, front to back (wave ballot + prefix popcount over the coarse bins): tile_count i32 [V,T] workspace,
 * tile_start i32 [V,T+2] ([0..T] clamped to cap_d, [T+1] = true pair count), ids i32 [V,cap_d] */
int siu3r_raster_tile_lists(const siu3r_raster_cam* cams_host, int V, const int32_t* bin_start, const void* entries, int64_t cap_e,
                            int32_t* tile_count, int32_t* tile_start, int32_t* ids, int64_t cap_d, uint64_t* stats, void* stream);
/* stage 4 (mode 1): feats [G,channels] -> out [V,H,W,channels] (+ alphas [V,H,W]) over the tile lists, 32 channels per pass (alpha and
 * transmittance re-evaluated per pass).  A pixel only ever sees the feature rows of entries that reach it with alpha >= 1/255.
 * An empty scene (G == 0; then rec / feats / ids may be null) renders zero maps. */
int siu3r_raster_composite_feat(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start,
                                const int32_t* ids, int64_t cap_d, const float* rec, const float* feats, int channels, float* out,
                                float* out_alpha, void* stream);
/* the same with a WORKSPACE (device, ws_bytes >= siu3r_raster_composite_feat_ws_bytes(width, height, V, cap_d), 4-byte aligned): for
 * channels >= 32 (arrays below 4 GiB) the tile lists are first cut per 8 x 8 pixel quadrant (a conservative footprint test; 16 * cap_d +
 * 16 * T bytes per view) and every wave of the composite walks its own quadrant's list with wave-private LDS staging, all channels in
 * one pass per 192-channel chunk, the blend as rank-2 v_mfma_f32_32x32x2_f32 updates (exact f32, accumulating in list order) -- no
 * workgroup barrier in the kernel.  Identical bits to siu3r_raster_composite_feat FOR FINITE FEATURES (which it falls back to without a
 * workspace, below 32 channels, or after siu3r_raster_tune(0, 1)).  Restriction: every pixel of a quadrant takes part in every entry of
 * the quadrant's list with weight 0 where the entry does not reach it, and list tails are padded with Gaussian 0's row, so a NON-FINITE
 * feature value (0 * inf = NaN) in any listed Gaussian -- or in Gaussian 0 -- poisons pixels the 32-channel kernel leaves untouched:
 * callers that may hold non-finite features select the 32-channel kernel (tests/test_raster_gpu.py pins both behaviours). */
int64_t siu3r_raster_composite_feat_ws_bytes(int width, int height, int V, int64_t cap_d);
/* 1 when siu3r_raster_composite_feat_ws takes the matrix-core form for these arguments (and so leaves the per-quadrant lists in ws, which a
 * backward may reuse), 0 when it falls back to the 32-channel kernel; evaluated with the current siu3r_raster_tune state */
int siu3r_raster_composite_feat_ws_lists(int width, int height, int V, int64_t G, const float* feats, int channels, const void* ws, int64_t ws_bytes,
                                         int64_t cap_d);
int siu3r_raster_composite_feat_ws(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start,
                                   const int32_t* ids, int64_t cap_d, const float* rec, const float* feats, int channels, float* out,
                                   float* out_alpha, void* ws, int64_t ws_bytes, void* stream);
/* tuning / A-B switches of the rasterizer (not for concurrent use).  key 0: 1 = the 32-channel kernel for every N-channel composite, 0 =
 * default (matrix-core form where it applies); key 1: accumulator blocks per chunk of the matrix-core form (1 .. 6, default 6) */
int siu3r_raster_tune(int key, int value);
/* per-Gaussian blend-contribution statistics (csrc/contrib.hip; an addition, ABI version unchanged).  Consumes the state of a forward
 * call (project -> sort -> bin) exactly as siu3r_raster_composite_rgb does and re-walks it without colours, either family (mode 0: pixel
 * centres at integers, saturation nT < t_min; mode 1: centres at +0.5, nT <= t_min; a mixed array is refused).  With w = alpha * T the very
 * float the forward adds into a pixel, over the pixels of view v that blend Gaussian g (reached, not the saturating entry):
 *   wmax  [V, G] fp32   the largest w (rows that blend nowhere stay exactly 0.0f)
 *   count [V, G] int32  the number of those pixels                                              (optional: NULL = not wanted)
 *   wsum  [V, G] uint64 the sum of (uint64_t)(w * 2^40): a fixed-point sum in units of 2^-40    (optional: NULL = not wanted)
 * All three are zeroed here and reduced with integer operations only (the maximum on the bit patterns of w >= 0), so they are
 * bit-reproducible.  A view whose coarse-bin entries overflowed (bin_start[v][NB] > cap_e) gets NaN in every element of its wmax row and
 * zeros in count and wsum.  G == 0 writes nothing and accepts null pointers; a null wmax with G > 0 is refused. */
int siu3r_raster_contrib(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start, const void* entries,
                         int64_t cap_e, const float* rec, float* wmax, int32_t* count, uint64_t* wsum, void* stream);
/* ---- K2 backward (mode 0 cameras only; additions of ABI 10, backward compatible).  The forward's state of the same call is reused:
 * cams_dev, bin_start, entries, cap_e, rec, rect and the outputs image [V,3,H,W] (with background), depth [V,H,W], alpha [V,H,W].
 * composite: upstream gradients g_image / g_depth / g_alpha (shapes of the outputs) -> grad [V, G, 10] fp32 (zeroed here) =
 * d loss / d {mean2d x, y, conic a, b, c, opacity, r, g, b, depth} of every (view, Gaussian) record; float atomics, one per
 * (tile, Gaussian, non-zero term) */
int siu3r_raster_composite_rgb_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                   const void* entries, int64_t cap_e, const float* rec, const float* image, const float* depth, const float* alpha,
                                   const float* g_image, const float* g_depth, const float* g_alpha, float* grad, void* stream);
/* the same launch with the absolute-gradient densification statistics of AbsGS (Ye et al. 2024; an addition, ABI version unchanged):
 * grad exactly as above, and abs_mean2d [V, G, 2] fp32 (zeroed here) = the sum over the pixels that blend the Gaussian of |that pixel's
 * mean2d x term| and |its mean2d y term| -- the absolute value is taken per pixel, before any sum, so contributions of opposite sign
 * from the two sides of a footprint do not cancel (|grad[.., 0..1]| <= abs_mean2d).  A pixel whose alpha sits on the alpha_max clamp
 * contributes 0, as to grad; rows of Gaussians that blend nowhere stay exactly 0.  Float atomics, one per (tile, Gaussian, non-zero
 * term).  Mode 0 cameras only (a mode-1 view array is refused); a null abs_mean2d is refused like a null grad (G == 0 writes nothing
 * and accepts both). */
int siu3r_raster_composite_rgb_bwd_abs(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                       const void* entries, int64_t cap_e, const float* rec, const float* image, const float* depth,
                                       const float* alpha, const float* g_image, const float* g_depth, const float* g_alpha, float* grad,
                                       float* abs_mean2d, void* stream);
/* projection: grad [V, G, 10] -> g_means [G,3], g_cov [G, cov_stride] (stride 9: entries 0, 1, 2, 4, 5, 8, zeros elsewhere), g_opacities
 * [G], g_colors (the layout and size of colors; sh_degree < 0: the precomputed [G,1,3] colours), summed over the views (no atomics);
 * g_mean2d [V, G, 2] optional (pixel-space mean gradient); pose_part optional: [siu3r_raster_pose_partial_rows(G), V, 6] per-workgroup
 * sums of d loss / d (rho, theta) of the left perturbation w2c <- exp(xi^) w2c (P moving with it), reduced by siu3r_raster_pose_reduce */
int siu3r_raster_project_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                             int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect,
                             const float* grad, float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d,
                             float* pose_part, void* stream);
/* the same for a forward that projected with siu3r_raster_project_aa / _c2w_aa (an addition, ABI version unchanged): the gradient of the
 * anti-aliased record on the branch the forward took.  g_opacities += comp * grad[OP]; where r = det0 / det1 > 2.5e-5,
 * d loss / d comp = grad[OP] * opacity goes through d comp / d r = 0.5 / comp and d r / d (c00', c01, c11') = (B / det1^2) (c11' c11 +
 * c01^2, -2 c01 (c00' + c11), c00' c00 + c01^2) (the quotient rule with det1 - det0 = B (c00' + c11' + B) cancelled by hand: sums of
 * like-signed terms) into the 2-D covariance gradient, added to the conic's contribution in front of the one
 * chain to the covariance, the Jacobian, the mean and the pose partial rows; on the floor comp is a constant and only the opacity term remains. */
int siu3r_raster_project_bwd_aa(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                int cov_stride, const float* opacities, const float* colors, int channels, int sh_planar, const int32_t* rect,
                                const float* grad, float* g_means, float* g_cov, float* g_opacities, float* g_colors, float* g_mean2d,
                                float* pose_part, void* stream);
int64_t siu3r_raster_pose_partial_rows(int64_t G);
/* pose_part [nrows, V, 6] -> g_pose [V, 6] = (rho, theta) per view */
int siu3r_raster_pose_reduce(int V, int64_t nrows, const float* pose_part, float* g_pose, void* stream);
/* ---- gsplat-family backward (mode 1 cameras only; additions of ABI 10, backward compatible).  The forward's state of the same call is
 * reused (cams_dev, rec, rect, bin lists / tile lists).  Gradients are those of the function the forward computes, on the branch it took.
 * three-channel fused path (siu3r_raster_composite_rgb with mode-1 cameras): colors [V,H,W,3] and alphas [V,H,W] as the forward wrote them
 * (no background), their upstream gradients -> grad [V, G, 10] (zeroed here; terms as siu3r_raster_composite_rgb_bwd, depth unused) */
int siu3r_raster_composite_rgb_bwd_k3(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* bin_start,
                                      const void* entries, int64_t cap_e, const float* rec, const float* colors, const float* alphas,
                                      const float* g_colors, const float* g_alphas, float* grad, void* stream);
/* the per-8 x 8-quadrant lists of the N-channel composite (what siu3r_raster_composite_feat_ws builds into its workspace for C >= 32), for
 * a backward whose forward ran without them; ws as siu3r_raster_composite_feat_ws (ws_bytes >= siu3r_raster_composite_feat_ws_bytes) */
int siu3r_raster_quad_lists(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start, const int32_t* ids,
                            int64_t cap_d, const float* rec, void* ws, int64_t ws_bytes, void* stream);
/* N-channel composite (either forward form: the quadrant lists give the same per-pixel walk): out [V,H,W,C], out_alpha [V,H,W], upstream
 * gradients g_out / g_alpha -> grad [V, G, 10] (terms 0..5) and g_feats [G, C] (both zeroed here; float atomics).  Features must be finite. */
int siu3r_raster_composite_feat_bwd(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const int32_t* tile_start,
                                    const void* ws, int64_t cap_d, const float* rec, const float* feats, int channels, const float* out,
                                    const float* out_alpha, const float* g_out, const float* g_alpha, float* grad, float* g_feats, void* stream);
/* projection: grad [V, G, 10] -> g_means [G,3], g_cov [G, cov_stride] (stride 9: entries 0, 1, 2, 4, 5, 8, zeros elsewhere), g_opacities
 * [G], g_colors [G,3] optional (the three-channel path's record colours), summed over the views; pose_part optional:
 * [siu3r_raster_pose_partial_rows(G), V, 12] per-workgroup sums of d loss / d [R | t] of each world->camera matrix */
int siu3r_raster_project_bwd_k3(const siu3r_raster_cam* cams_host, int V, const void* cams_dev, int64_t G, const float* means, const float* cov,
                                int cov_stride, const int32_t* rect, const float* grad, float* g_means, float* g_cov, float* g_opacities,
                                float* g_colors, float* pose_part, void* stream);
/* pose_part [nrows, V, 12] -> g_viewmats [V, 4, 4] (bottom row zero) */
int siu3r_raster_viewmat_reduce(int V, int64_t nrows, const float* pose_part, float* g_viewmats, void* stream);
/* x *= s in place (the reference rescales the scene x10 in place, src/models/gaussian_renderer.py:43-46) */
int siu3r_scale_inplace(float* x, int64_t n, float s, void* stream);
/* query-class-logit lifting (reference src/pipeline.py:137-193): rendered [V,H,W,q*C] -> sem_id, ins_id int64 [V,H,W];
 * first_pix [q] i32 workspace/out (first pixel owned by each query, or INT_MAX), q_label [q] i32 out */
int siu3r_lift_ids(const float* qc, int V, int H, int W, int q, int C, float sem_threshold, int num_queries,
                   uint32_t stuff_mask, int64_t* sem_id, int64_t* ins_id, int32_t* first_pix, int32_t* q_label,
                   void* stream);

/* fp32 [rows, k] (row stride ldx) -> bf16 hi plane [rows,kpad] (+ optional lo = bf16(x - hi)), zero padded:
 * weight / operand pre-packing for siu3r_gemm.  x3 (optional, kpad % 32 == 0): both planes interleaved per 32-deep K tile,
 * [rows][kpad / 32][hi 32 | lo 32] = siu3r_gemm_params.w_x3.  hi may be null when x3 is given. */
int siu3r_split_bf16(const float* x, void* hi, void* lo, void* x3, int64_t rows, int k, int kpad, int64_t ldx, void* stream);

/* ---- panoptic post-process on device (integer outputs).  Replaces
 * VideoMask2FormerImageProcessor.post_process_panoptic_segmentation
 * (reference src/models/mask2former/image_processing_video_mask2former.py:1238-1481) and the label scatter of
 * SIU3RModel.post_process_gaussians (reference src/models/model.py:267-294).
 * class_logits [B,Q,C] fp32; mask_logits_cl [B,T,IH,IW,Q] fp32 (channel-last).  All other pointers are outputs /
 * workspaces: probs [B,Q,C], scores [B,Q], labels/kept_idx [B,Q] i32, n_keep [B] i32, p256 [B,T,Q,ms,ms] fp32 (the ms x ms probability planes of the KEPT queries of an item: plane k < n_keep[b] belongs to query kept_idx[b,k]; the rest is not written),
 * lab_map [B,T,H,W] i32, area/orig [B,Q] i32, per-kept-query table seg_id/seg_label/seg_fused [B,Q] i32 + seg_score
 * [B,Q] fp32, acc_list [B,Q] / n_acc [B] i32, and the maps seg/sem/ins [B,T,H,W] i32.  fuse_mask bit c = class c fuses.
 * threshold and mask_threshold are compared in float32 (as torch compares a float32 tensor with a Python scalar); overlap is a DOUBLE: the
 * float32 quotient area / orig is widened and compared with it, as the reference compares `ratio.item()` with its Python float. */
int siu3r_panoptic_stage1(const float* class_logits, const float* mask_logits_cl, float* probs, float* scores,
                          int32_t* labels, int32_t* kept_idx, int32_t* n_keep, float* p256, int32_t* lab_map,
                          int32_t* area, int32_t* orig, int32_t* seg_id, int32_t* seg_label, int32_t* seg_fused,
                          float* seg_score, int32_t* acc_list, int32_t* n_acc, int32_t* seg, int32_t* sem, int32_t* ins,
                          int B, int T, int Q, int C, int IH, int IW, int H, int W, int mask_size, float threshold,
                          float mask_threshold, double overlap, uint32_t fuse_mask, void* stream);
/* query_class_logits of batch item b in Gaussian-major layout out[(t,y,x), j, c] (model.py:261-263) */
int siu3r_panoptic_qcl(const float* p256, const float* probs, const int32_t* kept_idx, const int32_t* acc_list, int nq,
                       float* out, int b, int T, int H, int W, int mask_size, int Q, int C, void* stream);

/* ---- viewer-semantics render helpers (reference viewer.py:301-336: gsplat.rasterization(means, quats, exp(scales), sigmoid(opacities),
 * colors = cat(sh0, shN), sh_degree, backgrounds = 1); gsplat is un-vendored: published algorithm, see oracle/raster_ref.c) ------------ */
/* quats (w,x,y,z, normalised here) + scales -> the 6 upper-triangular covariance entries consumed by siu3r_raster_bin */
int siu3r_quat_scale_to_cov6(const float* quats_wxyz, const float* scales, float* cov6, int64_t G, void* stream);
/* view-dependent colour: rgb[G,3] = max(SH_degree(normalise(mean - campos)) . sh[G,ncoef,3] + 0.5, 0); campos3_host is a HOST pointer */
int siu3r_sh_eval(const float* means, const float* campos3_host, const float* sh, int ncoef, int degree, float* rgb, int64_t G, void* stream);
/* colors[pixels, channels] += (1 - alpha[pixels]) * bg[channels]; bg_host is a HOST pointer, channels <= 3 */
int siu3r_blend_background(float* colors, const float* alpha, const float* bg_host, int channels, int64_t pixels, void* stream);
/* the two helpers with their small operand in DEVICE memory (no host round trip of a pose / background tensor): campos3_dev = 3 floats,
 * bg_dev = `channels` floats (any channel count) */
int siu3r_sh_eval_dp(const float* means, const float* campos3_dev, const float* sh, int ncoef, int degree, float* rgb, int64_t G, void* stream);
int siu3r_blend_background_dp(float* colors, const float* alpha, const float* bg_dev, int channels, int64_t pixels, void* stream);
/* backward passes of the two helpers: g_cov6 [G,6] -> g_quats [G,4] (through the normalisation), g_scales [G,3]; g_rgb [G,3] -> g_sh
 * [G,ncoef,3] (zero where a colour was clamped at 0 and past the degree), g_means [G,3] (through the view direction), g_campos3 [3] (device,
 * zeroed here) */
int siu3r_quat_scale_to_cov6_bwd(const float* quats_wxyz, const float* scales, const float* g_cov6, float* g_quats, float* g_scales, int64_t G, void* stream);
int siu3r_sh_eval_bwd(const float* means, const float* campos3_dev, const float* sh, int ncoef, int degree, const float* g_rgb, float* g_sh, float* g_means,
                      float* g_campos3, int64_t G, void* stream);

/* ---- photometric loss of splat refinement (csrc/photo_loss.hip): loss = (1 - lambda) * L1 + lambda * (1 - SSIM), value and gradient fused ----
 * pred / target: fp32 images of V views x C channels x H x W pixels, read AS STORED through four ELEMENT strides (view, channel, row,
 * column; host arrays of 4, >= 0), so that [V,C,H,W] and [V,H,W,C] are both consumed without a copy.  L1 = mean |pred - target| over all
 * pixels; SSIM = metrics.ssim with an explicit data_range (separable 11-tap Gaussian window, sigma 1.5, k1 0.01, k2 0.03, per channel,
 * variances clamped at 0) averaged over the valid region (H - 10) x (W - 10), then over channels and views.  lambda = 0 computes no SSIM,
 * lambda = 1 no L1 (the term left out is reported as NaN); every other lambda needs H, W >= 11.
 * grad_pred (or NULL): d loss / d pred in pred's layout (same strides; every pixel is written), for a loss gradient of 1; the subgradient
 * of |x| at 0 and the gradient through a clamped variance are 0.
 * partials: 2 * siu3r_photo_loss_partials(V, C, H, W) floats of workspace (one (L1, SSIM) pair of sums per workgroup); out: 3 floats on
 * the device = (loss, L1, SSIM).  Deterministic: fixed-order sums, no atomics; two calls on the same input give the same bits. */
int64_t siu3r_photo_loss_partials(int V, int C, int H, int W);
int siu3r_photo_loss(const float* pred, const float* target, int V, int C, int H, int W, const int64_t* pred_strides,
                     const int64_t* target_strides, float lambda, float data_range, float* grad_pred, float* partials, float* out,
                     void* stream);

/* ---- depth loss of splat refinement (csrc/depth_loss.hip): value and gradient w.r.t. the K2 render's depth and opacity ----
 * depth (D = sum w z), opacity (O = sum w), target (T), weight (Wt, or NULL = 1): fp32 [V,H,W], contiguous, on the device.
 * A pixel is valid iff O > min_opacity, D > 0, T > 0, Wt > 0 and all four are finite (a NaN fails every comparison); an invalid pixel
 * adds nothing to any sum and gets +0 in both gradient maps.  space 0: x = D / O against y = T; space 1: x = O / D against y = 1 / T.
 * mode 0 (l1): loss = sum w |x - y| / N, N = sum w over the valid pixels of all views (N = 0: loss 0); out = (loss, N, 1 / N or 0, 0);
 *   per_view [V] = the view's sum w |x - y| / sum w (NaN without a valid pixel).  g_depth / g_opacity are written WITHOUT the factor 1 / N:
 *   d loss / d depth = g_depth * out[2] (one pass; the caller folds out[2] into the multiply with its upstream gradient).
 * mode 1 (pearson): per view rho of the w-weighted (x, y) over its valid pixels; a view counts iff it has >= 2 valid pixels, max x > min x
 *   and max y > min y; loss = mean of 1 - rho over the counted views (none: 0); out = (loss, counted views, 1, 0); per_view [V] = 1 - rho
 *   (NaN for a view that is not counted); g_depth / g_opacity are the full derivative (zero in a view that is not counted).
 * valid [V] int32: the exact number of valid pixels per view.  g_depth, g_opacity: both [V,H,W] (every pixel is written) or both NULL.
 * ws: siu3r_depth_loss_ws(V, H, W) BYTES of workspace, 8-byte aligned (0: the shape is not supported).  H * W < 2^31 - 1024, V <= 65535,
 * min_opacity >= 0.  Deterministic (fixed-order fp64 sums, no atomics); nothing allocates or synchronises with the host. */
int64_t siu3r_depth_loss_ws(int V, int H, int W);
int siu3r_depth_loss(const float* depth, const float* opacity, const float* target, const float* weight, int V, int H, int W, int mode, int space,
                     float min_opacity, float* g_depth, float* g_opacity, void* ws, float* out, float* per_view, int32_t* valid, void* stream);

/* ---- instance-aware depth smoothness of splat refinement (csrc/depth_smooth.hip): value and gradient w.r.t. the K2
 * render's depth and opacity ----
 * depth (D = sum w z), opacity (O = sum w; may be NULL with space 0): fp32 [V,H,W]; segments: int32 [V,H,W] or NULL (one segment, nothing
 * void), any negative id is void; all contiguous, on the device.
 * space 0 (render): x = D, a pixel is usable iff D is finite.  space 1 (expected): x = D / O, usable iff O > min_opacity, D > 0 and both are
 * finite (the rule of siu3r_depth_loss).  Terms along x (along y: the axes swapped): order 1: t = x[j+1] - x[j], j = 0 .. W-2; order 2:
 * t = x[j-1] - 2 x[j] + x[j+1], j = 1 .. W-2.  A term is active iff all its pixels are usable, none is void and all carry the same id.
 * loss = Sx / n_x + Sy / n_y, S = sum |t| over the active terms, n_x = V H (W - order), n_y = V (H - order) W: the number of term POSITIONS
 * (inactive ones count as zeros); an axis without a position adds 0.  out = (loss, Sx / n_x, Sy / n_y, 0); per_view [V] = the view's two
 * parts, each over the view's own positions, summed; active [V,2] int32 = the exact number of active terms per view along x and along y.
 * g_depth, g_opacity: [V,H,W], the full derivative (sign(0) = 0), every pixel written exactly once, +0 at an unusable or void pixel; both
 * NULL: value only.  With space 0 g_opacity may be NULL (else it is written as zeros); with space 1 they come together.
 * ws: siu3r_depth_smooth_ws(V, H, W) BYTES of workspace, 8-byte aligned (0: the shape is not supported).  H * W < 2^31 - 1024, V <= 65535,
 * H <= 16 * 65535, min_opacity >= 0.  Deterministic (fixed-order fp64 sums, a gather, no atomics); nothing allocates or synchronises with
 * the host. */
int64_t siu3r_depth_smooth_ws(int V, int H, int W);
int siu3r_depth_smooth(const float* depth, const float* opacity, const int32_t* segments, int V, int H, int W, int order, int space,
                       float min_opacity, float* g_depth, float* g_opacity, void* ws, float* out, float* per_view, int32_t* active, void* stream);

/* ---- adaptive density control of splat refinement (csrc/density.hip; Kerbl et al. 2023, section 5.2): clone / split / prune ----
 * Deterministic (no float atomics; two calls on the same input give the same bits), nothing allocates or synchronises with the host.
 * Statistics, every iteration.  g_mean2d [V,G,2]: the pixel-space mean gradient as siu3r_raster_project_bwd writes it (rows of culled
 * Gaussians are never read: visibility is radii > 0); radii [V,G,2] i32.  For every view, in index order, with radii[v,g,0] > 0 or
 * radii[v,g,1] > 0:  grad_accum[g] += hypot(sx gx, sy gy), seen[g] += 1, max_radius[g] = max(max_radius[g], radii[v,g,:]).  The three
 * running arrays ([G] f32 / i32 / i32) are read and written. */
int siu3r_density_accumulate(const float* g_mean2d, const int32_t* radii, int V, int64_t G, float sx, float sy, float* grad_accum,
                             int32_t* seen, int32_t* max_radius, void* stream);
/* Plan.  action[g]: 0 prune (no output row), 1 keep (1), 2 clone (2), 3 split (2), from
 *   avg = seen > 0 ? grad_accum / seen : 0 (an fp64 quotient),  hot = avg >= grad_threshold,  big = max_k log_scales[g,k] > log_dense_scale,
 *   prune = logit_opacity[g] < logit_min_opacity  ||  (max_screen_radius > 0 && max_radius[g] > max_screen_radius)
 *           ||  max_k log_scales[g,k] > log_max_world_scale  (+infinity switches it off);
 *   prune -> 0, else hot && grow -> (big ? 3 : 2), else 1.
 * offset [G]: the exclusive scan of the output rows in memory order (rows of g: offset[g] .. offset[g] + rows - 1); totals [4] = rows out,
 * pruned, cloned, split; ws: siu3r_density_plan_ws(G) int32 of workspace.  All of these live on the device.  G <= 2^30. */
int64_t siu3r_density_plan_ws(int64_t G);
int siu3r_density_plan(const float* grad_accum, const int32_t* seen, const int32_t* max_radius, const float* log_scales,
                       const float* logit_opacity, int64_t G, float grad_threshold, float log_dense_scale, float logit_min_opacity,
                       int max_screen_radius, float log_max_world_scale, int grow, int32_t* action, int32_t* offset, int32_t* ws,
                       int32_t* totals, void* stream);
/* Apply, one call per field: gathers src [G,r] fp32 (and its Adam moments m1 / m2 [G,r], both or neither) into dst / dst_m1 / dst_m2
 * [rows out, r].  keep: the row's bits and moments; clone: the bits twice, the second row with zero moments; split: two rows with zero
 * moments, by mode:  0 the parent's bits;  1 (means, r = 3) mean + R(q / |q|) (exp(log_scales[g]) o noise[g,c,:]) for child c, with
 * quats_xyzw [G,4] raw (x, y, z, w), log_scales [G,3] and noise [G,2,3] (the caller's unit normals);  2 (log-scales, r = 3) - log(1.6).
 * The three extra inputs are read in mode 1 only.  G * r < 2^31. */
int siu3r_density_apply(int mode, const float* src, const float* m1, const float* m2, int r, int64_t G, const int32_t* action,
                        const int32_t* offset, const float* quats_xyzw, const float* log_scales, const float* noise, float* dst,
                        float* dst_m1, float* dst_m2, void* stream);

/* ---- fused visibility-aware Adam of splat refinement (csrc/gaussian_adam.hip): all fields in ONE launch ----
 * A field is a dense fp32 [G, width] array on the device with its gradient and its two Adam moments, all of that shape; bases need only be
 * 4-byte aligned (16-byte aligned bases take the 16-byte path).  The element with index i within its row steps with `lr` when
 * head_period == 0 or i % head_period == 0 and with `lr_tail` otherwise (harmonics [G,3,n], head_period = n: DC at lr, the rest at lr_tail). */
#define SIU3R_ADAM_MAX_FIELDS 8
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int32_t width;       /* floats per row, > 0 */
  int32_t head_period; /* >= 0 */
  float lr, lr_tail;   /* >= 0 */
} siu3r_adam_field;
/* fields: a HOST array of n_fields (1 .. SIU3R_ADAM_MAX_FIELDS) entries, copied into the kernel arguments (nothing is uploaded).
 * A visible row, in fp32 and in the operation order of torch.optim.Adam (amsgrad off, no weight decay):
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * (the betas are doubles so that 1 - beta is rounded to fp32 once)
 * with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t of the caller's GLOBAL step count t (computed in double, passed as floats), also for rows that
 * earlier calls skipped; this is this project's definition and is unverified against the sparse Adam of the 3DGS code base.  Non-finite
 * gradients propagate, nothing is special-cased.
 * Visibility, at most one of: radii [V,G,R] int32 (the K2 render's radii, R = 2: a row is visible iff any of its V * R entries is > 0;
 * reduced by a small launch of its own into ws, siu3r_gaussian_adam_ws(G) BYTES on the device) or mask [G] uint8 (non-zero = visible).
 * Both NULL: every row is visible and ws may be NULL.  An invisible row is not written (param, exp_avg, exp_avg_sq keep their bits) and its
 * grad is not read.  Elementwise and deterministic: two calls on equal inputs give equal bits.  Nothing allocates or synchronises with the
 * host.  Errors (a NULL pointer, width <= 0, more than 8 fields, a negative rate, both visibility forms): siu3r_last_error(). */
int64_t siu3r_gaussian_adam_ws(int64_t G);
int siu3r_gaussian_adam(const siu3r_adam_field* fields, int n_fields, int64_t G, double beta1, double beta2, float eps, float bc1, float bc2,
                        const int32_t* radii, int V, int R, const uint8_t* mask, void* ws, void* stream);

/* ---- MCMC densification of splat refinement (csrc/mcmc.hip; Kheradmand et al. 2024): relocate, grow, noise ----
 * All parameters are the UNCONSTRAINED ones of the refinement loop, fp32, contiguous, on the device: means [G,3], log-scales [G,3], raw
 * (x, y, z, w) quaternions [G,4], logit opacities [G].  1 <= G <= 2^30.  Deterministic (no float atomics; two calls on equal inputs give
 * equal bits), nothing allocates or synchronises with the host.  ws: siu3r_mcmc_ws(G) BYTES of workspace, 8-byte aligned.
 * Weights.  w[g] = (uint32) rint(sigmoid(a[g]) * 2^24), the sigmoid in fp64 (a NaN gives 0);  dead[g] = a[g] <= logit_min_opacity, an fp32
 * comparison.  relocate != 0: a dead row gets w = 0 (it is never drawn); relocate == 0 (growth): every row keeps its weight. */
int64_t siu3r_mcmc_ws(int64_t G);
int siu3r_mcmc_weights(const float* logit_opacity, int64_t G, float logit_min_opacity, int relocate, uint32_t* w, uint8_t* dead, void* stream);
/* Scan.  cum [G] = the inclusive scan of w in uint64 (total = cum[G - 1] < 2^54 for weights up to 2^24).  dead (or NULL: dead_idx and n_dead
 * are then not touched): dead_idx [G] receives the indices of the dead rows in memory order, n_dead (device) their number. */
int siu3r_mcmc_scan(const uint32_t* w, const uint8_t* dead, int64_t G, uint64_t* cum, int32_t* dead_idx, int32_t* n_dead, void* ws, void* stream);
/* Draws.  rbits [n] int64: the caller's random words, of which the low 32 bits r are used.  t = (r * total) >> 32, exact (the product has up
 * to 86 bits);  sampled[j] = the smallest g with cum[g] > t;  count [G] = how many of the n draws chose each row (cleared here).  All
 * integer: a pure function of (cum, rbits).  total == 0 (no row has a weight) makes every draw row 0.  0 <= n <= 2^32. */
int siu3r_mcmc_sample(const uint64_t* cum, int64_t G, const int64_t* rbits, int64_t n, int32_t* sampled, int32_t* count, void* stream);
/* Relocation update, in place, of every row with count[g] > 0, the row evaluated in fp64 and rounded once per output:
 *   N = min(count[g] + 1, 51);  o = sigmoid(a[g]);  o_new = 1 - (1 - o)^(1 / N);
 *   denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)   (summed over i first: sum_i C(i-1, k) = C(N, k+1));
 *   log_scales[g,:] += log(o / denom);  a[g] = logit(clamp(o_new, min_opacity, 1 - 1.1920929e-07)), the clamp after denom.
 * Rows with count[g] <= 0 keep their bits.  0 < min_opacity < 1. */
int siu3r_mcmc_relocate(float* log_scales, float* logit_opacity, const int32_t* count, int64_t G, double min_opacity, void* stream);
/* Row copy, one call per field [rows, r]: for j < n, field[d_j, :] = field[src[j], :] with d_j = dst[j], or G0 + j when dst is NULL (growth
 * into rows G0 .. G0 + n - 1 of a buffer whose first G0 rows the caller filled).  With moments (m1 / m2 [rows, r], both or neither) rows d_j
 * AND src[j] of both become zero: the source's moments belong to the Gaussian before its correction, the destination's to a Gaussian
 * that no longer exists (gsplat zeroes the sources only).  Sources and destinations are disjoint by construction and this is not
 * checked; an index outside 0 .. rows - 1 is skipped.  n >= 0, n * r < 2^31. */
int siu3r_mcmc_copy_rows(float* field, float* m1, float* m2, int r, int64_t rows, const int32_t* src, const int32_t* dst, int64_t G0, int64_t n,
                         void* stream);
/* Noise, in place on means, fp32:  o = sigmoid(a[g]);  gate = 1 / (1 + exp(-100 (gate_opacity - o)));
 *   means[g] += Sigma_g (noise[g] * gate * scaler),  Sigma_g = R(q / |q|) diag(exp(2 s)) R(q / |q|)^T,
 * R as in siu3r_density_apply mode 1; noise [G,3]: the caller's unit normals; quats_xyzw 16-byte aligned. */
int siu3r_mcmc_noise(float* means, const float* log_scales, const float* quats_xyzw, const float* logit_opacity, const float* noise, int64_t G,
                     float gate_opacity, float scaler, void* stream);
/* Regulariser lambda_o mean_g o + lambda_s mean_{g,k} exp(s[g,k]):  grad_opacity[g] += lambda_o o (1 - o) / G (the derivative by the logit),
 * grad_scales[g,k] += lambda_s exp(s[g,k]) / (3 G); either gradient may be NULL (a frozen field).  value [2] (device) = the two terms, by
 * fixed-order fp64 sums of the fp32 o and exp(s). */
int siu3r_mcmc_regularize(const float* logit_opacity, const float* log_scales, int64_t G, float lambda_o, float lambda_s, float* grad_opacity,
                          float* grad_scales, void* ws, float* value, void* stream);

/* ---- the cameras of splat refinement (csrc/camera.hip): per-view exposure and one fused pose / exposure step ----
 * Exposure.  out[v,c,p] = sum_k M[v,c,k] in[v,k,p] + M[v,c,3]: M [V,3,4] fp32 on the device, `in` fp32 images of V views x 3 channels x
 * H x W pixels read AS STORED through four ELEMENT strides (view, channel, row, column; a host array of 4, >= 0) as siu3r_photo_loss reads
 * its images, `out` contiguous [V,3,H,W].  An identity M returns the bits of a finite input (a -0 comes back as +0). */
int siu3r_exposure_apply(const float* in, const int64_t* in_strides, const float* M, int V, int H, int W, float* out, void* stream);
/* Backward from g_out (contiguous [V,3,H,W]); either output may be NULL (both NULL: nothing is launched).
 * g_in[v,k,p] = sum_c M[v,c,k] g_out[v,c,p], in in's layout (same strides; every pixel is written; the layout must not overlap itself).
 * g_M [V,3,4]: g_M[v,c,k] = sum_p g_out[v,c,p] in[v,k,p], g_M[v,c,3] = sum_p g_out[v,c,p]: exact fp64 products, fixed-order fp64 sums (per
 * workgroup, then the workgroups of a view in index order by a second launch), rounded once; ws: siu3r_exposure_ws(V, H, W) BYTES on the
 * device, 8-byte aligned (0: the shape is not supported), needed for g_M only.  H * W < 2^31 - 2048, V <= 65535.  Deterministic: no
 * atomics, two calls on equal inputs give equal bits.  Nothing allocates or synchronises with the host. */
int64_t siu3r_exposure_ws(int V, int H, int W);
int siu3r_exposure_apply_bwd(const float* in, const int64_t* in_strides, const float* M, const float* g_out, int V, int H, int W, float* g_in,
                             float* g_M, void* ws, void* stream);
/* Camera step: ONE launch, one thread per view, for the pose c2w [V,4,4] (camera-to-world, row-major) and the exposure M [V,3,4], both
 * updated in place.  Either half may be absent: c2w and g_xi both NULL, or M and g_M both NULL.  g_xi [V,6] = (rho, theta) = (translation,
 * rotation): the gradient of a LEFT perturbation of world->camera at 0, as the K2 backward returns it; g_M [V,3,4].
 * exp_avg / exp_avg_sq [V,18]: the Adam moments, 6 of the pose then 12 of the exposure.  free_mask [V] uint8 (or NULL: every view): a view
 * whose byte is 0 keeps the bits of c2w, M and its moments.  t >= 1: the caller's GLOBAL step count.
 * Per element, in fp64 from the fp32 state and rounded to fp32 once per stored value, in the operation order of siu3r_gaussian_adam:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + ((1 - beta2) g) g;  step = ((lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps),  bc = 1 - beta^t
 * with lr = lr_trans for rho, lr_rot for theta, lr_exposure for M (doubles: a host rate enters the fp64 arithmetic unrounded).  M -= step.  The pose variable is re-centred at 0 every step, so
 * xi = -step, and the pose is folded as c2w <- c2w exp(-xi^) (w2c <- exp(xi^) w2c), the exponential in closed form:
 *   exp(u^) = [R t; 0 1],  R = I + A K + B K^2,  t = (I + B K + C K^2) rho,  K = theta^,  th = |theta|,
 *   A = sin th / th,  B = (1 - cos th) / th^2,  C = (th - sin th) / th^3, each by its three-term series below th = 1e-2.
 * A free view whose six steps are exactly 0 (zero gradient and moments, eps > 0) keeps the bits of c2w.  R is not re-orthonormalised.
 * Elementwise and deterministic; nothing allocates or synchronises with the host.  Errors: siu3r_last_error(). */
int siu3r_camera_step(float* c2w, const float* g_xi, float* M, const float* g_M, float* exp_avg, float* exp_avg_sq, const uint8_t* free_mask, int V,
                      int64_t t, double lr_trans, double lr_rot, double lr_exposure, double beta1, double beta2, double eps, void* stream);

/* ---- bilateral-grid appearance correction of splat refinement (csrc/bilagrid.hip) ----
 * grids [V,12,L,Gh,Gw] fp32 on the device: per view a grid of 3 x 4 colour matrices, channel 4c + k = entry (c, k); 2 <= L <= 16,
 * 2 <= Gh, Gw <= 1024.  Slice: for pixel (y, x) of view v with colour p = (r, g, b),
 *   lum = 0.299 r + 0.587 g + 0.114 b,  fx = (x + 0.5) / W * (Gw - 1),  fy = (y + 0.5) / H * (Gh - 1),  fz = clamp(lum, 0, 1) * (L - 1),
 *   x0 = min(floor(fx), Gw - 2), tx = fx - x0 (likewise y, z),  M = the trilinear interpolation of the 8 corner matrices by nested
 *   a + t (b - a) steps (one fma each; x, then y, then z),  out[c] = M[c,0] r + M[c,1] g + M[c,2] b + M[c,3].
 * `in` is read AS STORED through four ELEMENT strides (view, channel, row, column; a host array of 4, >= 0) as siu3r_exposure_apply reads
 * its images, `out` is contiguous [V,3,H,W].  The identity grid (channels 0, 5, 10 one, the rest zero) returns the bits of a finite input
 * (a -0 comes back as +0); a NaN pixel gives a NaN output pixel and touches no other.  H * W < 2^31 - 2048, H, W <= 2^22, V <= 65535. */
int siu3r_bilagrid_apply(const float* in, const int64_t* in_strides, const float* grids, int V, int H, int W, int L, int Gh, int Gw, float* out,
                         void* stream);
/* Backward from g_out (contiguous [V,3,H,W]); either output may be NULL (both NULL: nothing is launched).
 * g_in, in in's layout (same strides; every pixel is written; the layout must not overlap itself):
 *   g_in[k] = sum_c M[c,k] g_out[c] + lw[k] (L - 1) [0 < lum < 1] sum_c g_out[c] (dM/dz [c,:] . (r, g, b, 1)),
 * dM/dz the xy-interpolated level z0 + 1 minus the xy-interpolated level z0; a clamped luminance gets no guidance gradient and the kink at an
 * integer fz is held constant (the kernel's own z0 decides).
 * g_grids [V,12,L,Gh,Gw], every element written: g_grids[v,4c+k,z,y,x] = sum over pixels of w_z w_y w_x g_out[c] (p_k or 1), gathered per
 * vertex in a fixed order (fp32 per thread, an fp64 tree per workgroup): no atomics, two calls on equal inputs give equal bits; a vertex no
 * pixel reaches gets exact zeros.  Nothing allocates or synchronises with the host. */
int siu3r_bilagrid_apply_bwd(const float* in, const int64_t* in_strides, const float* grids, const float* g_out, int V, int H, int W, int L, int Gh,
                             int Gw, float* g_in, float* g_grids, void* stream);
/* Total variation: value[0] = (1/V) sum_v sum_{axis in z, y, x} mean((A[.. i+1 ..] - A[.. i ..])^2), the mean per view over the 12 channels and
 * all positions of the differenced tensor: fp32 differences, fp64 products and fixed-order fp64 sums, rounded once.  g_grids (or NULL)
 * ACCUMULATES scale * d tv / d grids.  ws: siu3r_bilagrid_tv_ws(V, L, Gh, Gw) BYTES on the device, 8-byte aligned (0: the shape is not
 * supported).  Deterministic; nothing allocates or synchronises with the host. */
int64_t siu3r_bilagrid_tv_ws(int V, int L, int Gh, int Gw);
int siu3r_bilagrid_tv(const float* grids, int V, int L, int Gh, int Gw, float scale, float* g_grids, void* ws, float* value, void* stream);

/* ---- the 3-D smoothing filter of Mip-Splatting (csrc/mip_filter.hip; additions, ABI version unchanged) ----
 * filter [G]: the radius below which the training cameras cannot sample a Gaussian.  c2w_dev [V,4,4] camera-to-world (fourth row taken as
 * (0, 0, 0, 1)) and Kn_dev [V,3,3] NORMALISED intrinsics are row-major fp32 DEVICE tensors (no pose value is read on the host; the
 * world->camera rows are derived in fp64 and rounded once); width, height: the training frame; means [G,3].  With (x, y, z) the
 * camera-space point of a mean, fx, fy, cx, cy = Kn * (width, height), view v SEES the Gaussian when z > z_near and
 * fx x / z + cx lies in [-margin W, (1 + margin) W] and fy y / z + cy in [-margin H, (1 + margin) H] (the principal point is Kn's;
 * Mip-Splatting assumes the image centre).  d = the smallest z over the views that see it; a Gaussian no view sees (a NaN mean included)
 * takes the LARGEST d of the seen ones; focal = the largest fx over the views:
 *   filter = (sqrtf(variance) * d) / focal          (Mip-Splatting: z_near 0.2, margin 0.15, variance 0.2)
 * and all zeros when no view sees any Gaussian.  The largest d is a maximum over bit patterns: two calls give the same bits.
 * ws: siu3r_mip_filter3d_ws(V) BYTES on the device, 4-byte aligned.  z_near >= 0, margin >= 0, variance > 0.  Three launches; nothing
 * allocates or synchronises with the host.  G == 0 writes nothing. */
int64_t siu3r_mip_filter3d_ws(int V);
int siu3r_mip_filter3d(const float* c2w_dev, const float* Kn_dev, int V, int width, int height, const float* means, int64_t G, float z_near,
                       float margin, float variance, float* filter, void* ws, void* stream);
/* the filter applied to ACTIVATED scales [G,3] and opacities [G] (one launch):
 *   scales_f[i] = sqrtf(s_i^2 + f^2),   opac_f = o * (q_0 * q_1) * q_2,   q_i = |s_i| / scales_f[i]   (= sqrt(s_i^2 / (s_i^2 + f^2)); 1 where
 * s_i = f = 0): the ratio is formed per axis, neither prod s_i^2 nor prod (s_i^2 + f^2) is.  scales_f must not alias scales. */
int siu3r_mip_apply(const float* scales, const float* opacities, const float* filter, int64_t G, float* scales_f, float* opac_f, void* stream);
/* its backward (one launch): g_scales[i] = g_scales_f[i] s_i / scales_f[i] + g_opac_f o (prod_{j != i} q_j) sign(s_i) (f / scales_f[i])^2 /
 * scales_f[i] (0 where scales_f[i] = 0), g_opac = g_opac_f (q_0 * q_1) * q_2.  The filter gets no gradient. */
int siu3r_mip_apply_bwd(const float* scales, const float* opacities, const float* filter, const float* g_scales_f, const float* g_opac_f, int64_t G,
                        float* g_scales, float* g_opac, void* stream);

#ifdef __cplusplus
}
#endif
#endif
