// Host-side launch prototypes of every HIP kernel in libladi_native (internal header).
// All activations are NHWC fp16 unless noted; every launcher is asynchronous on `st`, allocates
// nothing and is therefore hipGraph-capturable. Return 0 on success, negative on argument errors.
#pragma once
#include "common.h"

// ---- igemm.hip
// a.stats (optional): per-channel partial statistics of the output, [ceil(P / px)][Q][2] floats (sum, sumsq) where px =
// *stats_row_px pixels per row (a multiple of 32 chosen with the tile shape; 0 = not produced, use ladi_launch_gn_partial)
// ws / ws_bytes: caller-owned split-K slab (fp32 partial tiles) of at least ladi_igemm_splitk_ws_bytes(a, batch) bytes; null -> a
// process-wide grow-only fallback buffer (never freed, so pointers baked into captured graphs stay valid)
// sk_cnt: caller-owned arrival counters of the in-launch split-K combine (>= 1024 ints, zero-initialised once; every launch leaves them
// zeroed) -- one buffer per stream that may run split-K launches concurrently; null -> a process-wide buffer (single-stream callers)
int ladi_launch_igemm(const IGemmArgs& a, int batch, int cfg, hipStream_t st, int* stats_row_px = nullptr, float* ws = nullptr,
                      size_t ws_bytes = 0, int* sk_cnt = nullptr);
// text of the last rc -20 refusal (the span guard of igemm.hip): P, HsWs, ld and the span that reached the limit
const char* ladi_igemm_span_refusal();
// worst-case split-K slab for this problem over every admissible split configuration (0: split-K can never be chosen); depends on
// the problem shape only, so a planning pass and the real pass allocate identically
size_t ladi_igemm_splitk_ws_bytes(const IGemmArgs& a, int batch);

// ---- igemm8.hip (phase-staggered 8-wave large-tile kernel), igemm_lc.hip (loader / consumer kernel), igemm_halo_inst_*.hip (halo-resident 3x3
// convolution) and igemm_inst_*.hip (ring kernel) define one launcher ladi_igemm_launch_base_<id>(IGemmArgs, int batch, hipStream_t) per row of
// igemm_tiles.h; igemm.hip, the only caller, declares them from the same rows and sets a.splitk / a.tile_map

// ---- igemm_halo.hip: what the halo-resident 3x3 convolution forms accept
bool ladi_igemm_halo_eligible(const IGemmArgs& a, int batch);              // ring-halo forms: rows of at most 48 pixels
bool ladi_igemm_halo2d_eligible(const IGemmArgs& a, int batch, int th);    // 2-D blocked forms: W % 32 == 0, H % th == 0
bool ladi_igemm_halo_ups_eligible(const IGemmArgs& a, int batch, int bp);  // folded nearest-2x upsample + 3x3 (round 6): whole bp-pixel tiles inside a sample

// ---- linear_xs.hip: X-stationary kernel for 1x1 layers with K = 320 / 640 (reached through ladi_launch_igemm cfg 23..27)
// nst: weight-ring depth (3: two workgroups per CU; 2: three workgroups per CU, K = 320 plain / GEGLU projections only)
bool ladi_linear_xs_eligible(const IGemmArgs& a, int batch, int pb, int qs, int nst = 3);
int ladi_launch_linear_xs(const IGemmArgs& a, int pb, int qs, hipStream_t st, int nst = 3);
void ladi_linear_xs_symbol(const IGemmArgs& a, int pb, int nst, char* out, int n);

// ---- xf_fused.hip: fused transformer sub-blocks of the C = 320 level (5 heads of 64); see the file header for the operand packings
struct XAttnBlockArgs {
    const h16* x; const h16* ln_g; const h16* ln_b; float ln_eps;     // block input [P][320] (dense rows), LayerNorm (norm2)
    const h16* Wq;                               // attn2.to_q [320][320] row-major, no bias
    const h16* Kp; const h16* Vt;                // packed context tiles of the FIRST sample of x: [n][5][96][68], [n][5][64][100]
    const h16* Wo; const h16* bo;                // attn2.to_out.0 packed [5][320][68], bias [320]
    const h16* res;                              // residual [P][320] (normally == x)
    h16* out;                                    // [P][320]
    int P, T, nk; float scale;                   // pixels, pixels per sample (multiples of 128), context length (<= 96), 1 / sqrt(64)
};
struct FFBlockArgs {
    const h16* x; const h16* ln_g; const h16* ln_b; float ln_eps;     // block input [P][320], LayerNorm (norm3)
    const h16* W1; const h16* b1;                // ff.net.0.proj in the GEGLU packing [2560][320], [2560] (load_geglu)
    const h16* W2; const h16* bo;                // ff.net.2 packed [40][320][36], bias [320]
    const h16* res;                              // residual [P][320] (normally == x)
    h16* out;
    int P;
};
bool ladi_xf_fused_eligible(int C, int heads, int T, int L);
size_t ladi_xf_kp_elems(int n);
size_t ladi_xf_vt_elems(int n);
size_t ladi_xf_wo_packed_elems();
size_t ladi_xf_w2_packed_elems();
int ladi_launch_pack_kv_tiles(const h16* kv, int n, int L, int C, h16* kp, h16* vt, hipStream_t st);   // kv [n][L][2C]
int ladi_launch_pack_wo(const h16* Wo, h16* out, hipStream_t st);
int ladi_launch_pack_w2(const h16* W2, h16* out, hipStream_t st);
int ladi_launch_xattn_block(const XAttnBlockArgs& a, hipStream_t st);
int ladi_launch_ff_block(const FFBlockArgs& a, hipStream_t st);        // LADI_FF_PIPE=0: the plain loop (A/B)

// ---- norm.hip
// GroupNorm in three stages (all atomics-free): per-channel partial statistics rows [rows][C][2] (written by the producing
// igemm's epilogue, or by ladi_launch_gn_partial), finalize -> scale_shift[n][C0+C1][2], apply.
int ladi_gn_partial_rows(int n, int HW, int C);   // rows per sample ladi_launch_gn_partial writes
int ladi_launch_gn_partial(const h16* src, int C, int ld, int n, int HW, float* part, hipStream_t st);
int ladi_launch_gn_finalize(const float* part0, int C0, int rps0, const float* part1, int C1, int rps1, int n, int HW, int groups,
                            const h16* gamma, const h16* beta, float eps, float* scale_shift, hipStream_t st, int* bad = nullptr);
// `bad` (optional, device): set to 1 when a group's statistics are not finite -- an fp16 overflow upstream (VAE range guard)
// y = act(x * scale + shift) (+ add) over the virtual concat (src0[C0] | src1[C1]): out [n][HW][C0+C1] dense
int ladi_launch_gn_apply(const h16* src0, int C0, int ld0, const h16* src1, int C1, int ld1, int n, int HW,
                         const float* scale_shift, int silu, const h16* add, h16* out, hipStream_t st);
// one-pass form (round 5): every block finalises the groups of its own 64-channel chunk from the partial rows (few rows per sample only:
// ladi_gn_norm_eligible) and applies -- no gn_finalize launch, no scale / shift table
// (rps = 0 with a null part pointer: that source has no partial rows and the kernel sums the data itself -- samples of <= 64 pixels only,
// ladi_gn_norm_direct)
// round 6: fold the many partial rows of a VAE-sized tensor ([n][rps][C][2]) into ladi_gn_reduce_rows() rows per sample ([n][rows][C][2]),
// after which ladi_launch_gn_norm takes it (rps > the one-pass kernel's row limit only)
int ladi_gn_reduce_rows();
bool ladi_gn_reduce_eligible(int C, int rps);
int ladi_launch_gn_reduce(const float* part, int C, int rps, int n, float* out, hipStream_t st);
bool ladi_gn_norm_direct(int HW);
bool ladi_gn_norm_eligible(int C0, int rps0, int C1, int rps1, int groups, int HW);
int ladi_launch_gn_norm(const h16* src0, int C0, int ld0, const float* part0, int rps0, const h16* src1, int C1, int ld1, const float* part1,
                        int rps1, int n, int HW, int groups, const h16* gamma, const h16* beta, float eps, int silu, const h16* add, h16* out,
                        hipStream_t st, int* bad = nullptr);
int ladi_launch_layernorm(const h16* x, int ldx, const h16* gamma, const h16* beta, float eps, int rows, int C, h16* out,
                          int ldo, hipStream_t st);
// P[r][:] = softmax(scale * S[r][:]) ; S fp32 [rows][cols], P fp16
int ladi_launch_softmax_rows(const float* S, int rows, int cols, float scale, h16* P, hipStream_t st);

// ---- attention.hip
struct AttnArgs {
    const h16* q; const h16* k; const h16* v; h16* o;
    int ldq, ldk, ldv, ldo;                 // row strides (elements)
    long long sq, sk, sv, so;               // per-sample strides (elements)
    int n, heads, Nq, Nk;                   // head h lives at column offset h*64 of each row
    float scale;
    int causal = 0;                         // 1: query i sees keys <= i (Nq == Nk)
    int qtiles = 0, xcd_map = 0;            // set by the launcher: query tiles per (sample, head); XCD-aware workgroup order
};
int ladi_launch_flash_attn64(const AttnArgs& a, hipStream_t st);
// heads of dimension 64 / 80 / 96 / 128 at column offset h*head_dim (CLIP ViT-H vision tower: 80); non-causal
int ladi_launch_attn_generic(const AttnArgs& a, int head_dim, hipStream_t st);
// ONE wide head (head_dim 128 / 256 / 512: the VAE AttentionBlock), flash-style; a.v = V^T [head_dim][Nk] (row stride a.ldv),
// a.heads must be 1, Nk % 4 == 0
int ladi_launch_attn_wide(const AttnArgs& a, int head_dim, hipStream_t st);
// single query per (sample, head): q [n][ldq], k/v [n][Nk][ld], generic head dim d <= 128
int ladi_launch_attn_single_query(const h16* q, int ldq, const h16* k, int ldk, const h16* v, int ldv, h16* o, int ldo,
                                  int n, int heads, int d, int Nk, long long sk, long long sv, float scale, hipStream_t st);

// ---- elementwise.hip
// out[m][nn] = act(sum_k x[m][k] W[nn][k] + b[nn]) for small M (weight-streaming GEMV-like); x/out fp16 or fp32
// optional residual res[m][nn] (fp16, row stride ldr) is added after the activation
int ladi_launch_small_linear(const void* x, int x_f32, int ldx, const h16* W, const h16* bias, const h16* res, int ldr, int M,
                             int N, int K, int act, int pre_silu, void* out, int out_f32, int ldo, hipStream_t st);
int ladi_launch_nchw_to_nhwc(const void* src, int src_f32, int n, int C, int H, int W, h16* dst, int ld, hipStream_t st);
int ladi_launch_nhwc_to_nchw(const h16* src, int ld, int n, int C, int H, int W, void* dst, int dst_f32, hipStream_t st);
// sinusoidal timestep embedding (flip_sin_to_cos=True, freq_shift=0): out[i][dim] fp32 for timesteps t[i]
int ladi_launch_timestep_embedding(const float* t, int count, int dim, float* out, hipStream_t st);

struct StepTable {            // one entry per scheduler evaluation, device resident (see sched.h)
    float c_x;                // multiplies current sample
    float c_e;                // multiplies the (possibly multistep-combined) epsilon
    float w[4];               // PLMS combination weights over [eps_now, ets[-1], ets[-2], ets[-3]]
    int   mode;               // 0 plain (use w), 1 = PLMS 2nd evaluation (eps'=(eps+ets[-1])/2, sample=cur_sample, no push),
                              // 2 = DPM-Solver++: the ring holds data predictions m = p_x * sample + p_e * eps, and w combines those
    int   push;               // bit0: push eps_now into the ring; bits 4-5: slot to push into;
                              // bits 8-9 / 10-11 / 12-13: ring slots holding ets[-1] / ets[-2] / ets[-3] (before the push)
    int   save_cur;           // 1: save current sample as cur_sample before the update
    int   zero_cloth_next;    // 1: the NEXT evaluation must see zero cloth latents
    float in_scale_next;      // scheduler.scale_model_input of the NEXT evaluation: the UNet sees latents * in_scale_next (1 for DDIM / PNDM,
                              // 1 / sqrt(sigma^2 + 1) for LMS); the fp32 latents themselves stay unscaled
    float p_x, p_e;           // mode 2: data prediction m = p_x * sample + p_e * eps (1 / alpha_s, -sigma_s / alpha_s)
    float c_n;                // multiplies this evaluation's step noise (Euler-ancestral sigma_up, DDIM-eta std; 0 = no noise term)
};
struct StepArgs {
    const h16* eps; int ld_eps;     // UNet output NHWC [2B or B][hw][ld_eps], channels 0..3 valid
    int B, hw, cfg;                 // cfg: 1 = rows [0,B) uncond, [B,2B) cond
    float guidance;
    float* latents;                 // fp32 [B][hw][4] in/out
    float* cur_sample;              // fp32 [B][hw][4] (PLMS)
    float* ets;                     // fp32 [4][B][hw][4] ring (PLMS); slot = (count) & 3
    const StepTable* table; int* step_idx;   // device step counter (read, then incremented by the kernel)
    h16* unet_in; int ld_in;        // next UNet input [2B or B][hw][ld_in]; channels 0..3 rewritten
    int cloth_ch0;                  // first cloth channel (27) ; zeroed when table says so (4 channels)
    // optional per-evaluation trace (parity tests): guided noise prediction and updated latents of evaluation i are written to
    // trace_*[i][B][hw][4] (fp32) for i < trace_cap; null = off
    float* trace_eps; float* trace_lat; int trace_cap;
    // per-evaluation noise (Euler-ancestral, DDIM with eta > 0): fp32 NCHW [evals][B][4][hw], indexed by the device step counter; read only where the
    // table's c_n != 0 (null = none)
    const float* step_noise;
    // per-evaluation guidance (all null = the scalar path above, bit for bit).  guidance_tab: device fp32 [evals], indexed by the device step
    // counter, replaces `guidance`; with cfg set, an entry <= 1 makes that evaluation cond-only: e is the conditional row [B, 2B) alone, the
    // uncond row of eps is not read (both halves of unet_in are still refreshed).  factor: device fp32 [B] of ladi_launch_cfg_stats for this
    // evaluation, multiplied into the guided e of a CFG evaluation before anything uses it (cond-only evaluations ignore it)
    const float* guidance_tab;
    const float* factor;
    // preserve-unmasked latent blend (all null = the code path above, bit for bit).  keep_mask fp32 [B][hw]: non-zero = a keep pixel; after the
    // update of evaluation i its latents are replaced by keep_tab[i][0] * keep_x0 + keep_tab[i][1] * keep_noise (both fp32 [B][hw][4]; keep_tab
    // device fp32 [evals][2], indexed by the device step counter; the row (1, 0) stores keep_x0 itself).  A select: the other pixels keep their
    // bits, and a keep pixel never sees eps.  The ring, cur_sample and the eps trace are not blended; trace_lat and unet_in get the blended value
    const float* keep_x0; const float* keep_noise; const float* keep_mask; const float* keep_tab;
    // perturbed-attention guidance (null = the code path above, bit for bit).  pag_tab: device fp32 [evals], indexed by the device step
    // counter.  An evaluation with s = pag_tab[i] > 0 has a third sample group p behind the cond group, rows [(cfg ? 2 : 1) * B, ..+B) of eps,
    // and its combine gains s (c - p): u + g (c - u) + s (c - p) with cfg, c + s (c - p) without or in a cond-only evaluation (which reads c
    // and p only).  `factor` multiplies the three-term sum.  With a table, eps and unet_in have the third group's rows whatever s is: the
    // refresh of unet_in (and the cloth zeroing) writes them too; an evaluation with s = 0 never reads the third group of eps
    const float* pag_tab;
    // self-attention guidance (null = the code path above, bit for bit; never together with pag_tab).  sag_scale: ONE device fp32, read by
    // every evaluation.  With s = *sag_scale != 0 the prediction d of the degraded input stands in the rows behind the last group,
    // [(cfg ? 2 : 1) * B, ..+B) of eps, and the combine gains s (b - d) with b the base prediction: u in a CFG evaluation, c without CFG or
    // in a cond-only evaluation.  `factor` multiplies the whole sum.  s = 0 never reads those rows
    const float* sag_scale;
};
int ladi_launch_sched_step(const StepArgs& a, hipStream_t st);
// guidance rescale statistics of one evaluation: eps as in StepArgs with cfg = 1 (rows [0,B) uncond, [B,2B) cond, row stride ld_eps halves, a
// multiple of 4; lanes 4.. are never read), g = guidance_tab[*step_idx] (both device) or, with a null table, `guidance`.  Writes
// factor[b] = phi * std(cond_b) / std(u_b + g (c_b - u_b)) + (1 - phi), unbiased stds over the 4 * hw elements of sample b, fp32, no epsilon.
// Fixed-order reduction (one workgroup per sample): bit-reproducible across launches and graph replays
int ladi_launch_cfg_stats(const h16* eps, int ld_eps, int B, int hw, const float* guidance_tab, const int* step_idx, float guidance,
                          float phi, float* factor, hipStream_t st);
// the same with perturbed-attention guidance: s = pag_tab[*step_idx] (device) or, with a null table, pag_scale; with s > 0 the guided
// prediction is u + g (c - u) + s (c - p), p the rows [2B, 3B) of eps; with s = 0 those rows are not read and the result is
// ladi_launch_cfg_stats' bit for bit.  Same two passes, same fixed-order sums
int ladi_launch_cfg_stats_pag(const h16* eps, int ld_eps, int B, int hw, const float* guidance_tab, const int* step_idx, float guidance,
                              const float* pag_tab, float pag_scale, float phi, float* factor, hipStream_t st);
// the same with self-attention guidance: s = *sag_dev (device) or, with a null pointer, sag_scale; with s != 0 the guided prediction is
// u + g (c - u) + s (u - d), d the rows [2B, 3B) of eps; with s = 0 those rows are not read and the result is ladi_launch_cfg_stats' bit for bit
int ladi_launch_cfg_stats_sag(const h16* eps, int ld_eps, int B, int hw, const float* guidance_tab, const int* step_idx, float guidance,
                              const float* sag_dev, float sag_scale, float phi, float* factor, hipStream_t st);

// static part of the 31-channel UNet input: mask, masked-image latents, pose, cloth; uncond half zero pose/cloth
int ladi_launch_assemble_static(h16* unet_in, int ld_in, int B, int hw, int cfg, const float* latents, const h16* mask_lat,
                                const float* masked_lat, const h16* pose, int pose_ch, const float* cloth_lat, int has_cloth,
                                float lat_scale, hipStream_t st, int pag = 0);     // pag: a third group of B samples, a copy of the cond group
// posterior sample: lat[b][hw][4] = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scaling ; moments NHWC [..][ldm] (8 ch),
// noise fp32 NCHW [B][4][h][w]; a null noise is the mode form: lat = mean * scaling
int ladi_launch_posterior_sample(const h16* moments, int ldm, const float* noise_nchw, int B, int hw, float scaling, float* lat,
                                 hipStream_t st);
// mask binarise (>=0.5 -> 1) at full res + masked image: img NHWC (ld) *= (mask<0.5); also writes binarised mask fp16 [B][H*W]
int ladi_launch_prepare_mask(const void* image_nchw, int img_f32, const void* mask_nchw, int mask_f32, int B, int H, int W,
                             h16* masked_img, int ld, h16* mask_bin, hipStream_t st);
// nearest downsample by integer factor s (top-left pixel): dst[b][h/s][w/s]
int ladi_launch_mask_down(const h16* src, int B, int H, int W, int s, h16* dst, hipStream_t st);
// bilinear /8 (align_corners=False == mean of centre 2x2) of pose [B][C][H][W] (NCHW) -> NHWC fp16 [B][h*w][C]
int ladi_launch_pose_down8(const void* pose_nchw, int f32, int B, int C, int H, int W, h16* dst, hipStream_t st);
// image = clamp(x/2+0.5, 0, 1) : src NHWC fp16 (ld) 3 valid channels -> fp32 [B][H][W][3], or (dst_u8) uint8 = round(image * 255)
int ladi_launch_image_post(const h16* src, int ld, int n_pix, void* dst, int dst_u8, hipStream_t st);
// features[i] *= (1-mask) standalone (mask_features for the module-by-module shim path)
int ladi_launch_mask_mul(h16* feat, int C, int n_pix, const h16* mask, hipStream_t st);
// one wave spins for wall_ticks ticks of the 100 MHz counter; out2 (device) = {shader cycles, wall ticks}
int ladi_launch_clock_probe(unsigned long long wall_ticks, unsigned long long* out2, hipStream_t st);
int ladi_launch_fill_f32(float* p, size_t n, float v, hipStream_t st);
int ladi_launch_scale_h16(const h16* src, int lds_, h16* dst, int ldd, size_t n_pix, int C, float s, hipStream_t st);
// CLIP text embeddings + pseudo-word splice: ids [B][T] (device), first [B] = position of the sentence's first '$' or -1,
// wemb fp16 [B][nv][H] or null; out [B][T][H] = (token | pseudo-word) embedding + position embedding
int ladi_launch_text_embed(const int* ids, const int* first, int nv, const h16* tok, const h16* pos, const h16* wemb, int B, int T,
                           int H, int vocab, h16* out, hipStream_t st);
// per sentence: first[b] = position of the first `vstar` id (or -1; -1 too when use_words == 0), eot[b] = b*T + argmax(ids[b]) (first maximum)
int ladi_launch_text_meta(const int* ids, int B, int T, int vstar, int use_words, int* first, int* eot, hipStream_t st);
// TPS matching network helpers: per-channel affine (BatchNorm after ReLU), per-pixel L2 normalisation over channels, TPS grid
int ladi_launch_channel_affine(const h16* x, int ldx, size_t n_pix, int C, const float* scale, const float* shift, h16* y, int ldy, hipStream_t st);
int ladi_launch_l2norm_rows(const h16* x, int ldx, int rows, int C, h16* y, int ldy, hipStream_t st);
// coor [B][N][2], inv [(N+3)^2], ctrl [N][2] (all fp32, device) -> grid [B][H][W][2] fp32
int ladi_launch_tps_grid(const float* coor, const float* inv, const float* ctrl, int N, int B, int H, int W, float* grid, hipStream_t st);
// refinement UNet helpers (NHWC fp16, C % 8 == 0): 2x2 max pooling; bilinear x2 upsampling with align_corners=True
int ladi_launch_maxpool2(const h16* src, int lds_, int n, int H, int W, int C, h16* dst, int ldd, hipStream_t st);
int ladi_launch_upsample2x_bilinear_ac(const h16* src, int lds_, int n, int H, int W, int C, h16* dst, int ldd, hipStream_t st);
// glue of the warping module (src/inference.py:242-260), NCHW planes, fp32 or fp16 in / out:
// torchvision resize(BILINEAR, antialias=True) == aten _upsample_bilinear2d_aa (align_corners=False)
struct ResizeEpi { int on, C; float pre_mul, pre_add; float sub[4], div[4]; float quant; };   // value epilogue, see elementwise.hip (quant > 0: floor(v * quant) / quant after the clamp)
int ladi_launch_resize_bilinear_aa(const void* src, int in_f32, int planes, int H, int W, void* dst, int out_f32, int Ho, int Wo,
                                   hipStream_t st, const ResizeEpi* epi = nullptr);
// F.grid_sample(x, grid, bilinear, padding_mode="border", align_corners=False); grid fp32 [B][Ho][Wo][2] (x, y)
int ladi_launch_grid_sample_border(const void* src, int in_f32, int B, int C, int H, int W, const float* grid, int Ho, int Wo, void* dst,
                                   int out_f32, hipStream_t st);
// ViT patch rows for the patch-embedding GEMM: out [B][1 + (S/ps)^2][KP] fp16, row 0 and the padding columns zero
int ladi_launch_patchify(const void* px, int in_f32, int B, int S, int ps, int KP, h16* out, hipStream_t st);
int ladi_launch_gather_rows(const h16* src, const int* rows, int n, int H, h16* dst, hipStream_t st);
// decoder input: post_quant_conv(lat / scaling_factor) -> NHWC fp16 padded to ld; pq = device [16 w | 4 b] or null (identity)
int ladi_launch_post_quant(const float* lat, const float* pq, float inv_sf, int n, h16* dst, int ld, hipStream_t st);
int ladi_launch_lat_nchw_to_pix(const float* src, int B, int hw, float scale, float* dst, hipStream_t st);
int ladi_launch_lat_pix_to_nchw(const float* src, int B, int hw, float* dst, hipStream_t st);
// start latents of a run that begins at an intermediate step: dst [B][h*w][4] = k_x * resample(init [B][4][hs][ws]) + k_n * noise [B][4][h][w]
// (fp32; bilinear, align_corners = False, no antialias; equal sizes: the samples themselves).  noise may be null when k_n == 0.  Returns -1
// for a null init / dst, a size < 1, or a null noise with k_n != 0
int ladi_launch_init_latents(const float* init, int hs, int ws, const float* noise, int B, int h, int w, float k_x, float k_n, float* dst,
                             hipStream_t st);
// step-callback import: fp32 NCHW [B][4][hw] src -> the loop's latents [B][hw][4], and the latent channels 0-3 of the next UNet input
// (rows [B] or, with cfg, [2B], ld_in halves per row) rewritten as fp16(x * in_scale) -- what sched_step_kernel wrote from the unedited x
// pag: the perturbed group's rows (behind the cond group's) are rewritten too
int ladi_launch_latents_import(const float* src, int B, int hw, float* latents, h16* unet_in, int ld_in, int cfg, float in_scale, hipStream_t st,
                               int pag = 0);
// preserve-unmasked.  mask_pool8: dst fp32 [B][H/8][W/8] = max over each 8x8 block of the binarised fp16 mask [B][H][W] (F.max_pool2d(mask, 8)),
// with `invert` 1 - that (the keep mask of StepArgs); H, W multiples of 8, mask 16-byte aligned, else -1
int ladi_launch_mask_pool8(const h16* mask_bin, int B, int H, int W, int invert, float* dst, hipStream_t st);
// separable Gaussian blur of the binarised fp16 mask [B][H][W] -> dst fp32 [B][H][W]: radius ceil(3 sigma), weights normalised in float64 on the
// host, replicate border, fp32 sums in the order k = -r .. r, two launches (rows into tmp fp32 [B][H][W], then columns).  -2: sigma outside (0, 32]
int ladi_launch_mask_feather(const h16* mask_bin, int B, int H, int W, float sigma, float* tmp, float* dst, hipStream_t st);
int ladi_feather_radius(float sigma);
// composite decode epilogue: dst [B*HW][3] (fp32, or u8 = round(255 v) as image_post) = M g + (1 - M) p, g = clamp(src / 2 + 0.5, 0, 1) from the
// decoded NHWC fp16 src (ld % 4 == 0), p the same of the NCHW image (fp32 / fp16), M fp16 or fp32 [B][HW]; M == 0 / 1 select p / g bit for bit.
// HW % 4 == 0 (else -1); 16-byte accesses where the pointers are aligned to them, element accesses otherwise
int ladi_launch_image_composite(const h16* src, int ld, const void* image_nchw, int img_f32, const void* mask, int mask_f32, int B, int HW,
                                void* dst, int dst_u8, hipStream_t st);

// ---- freeu.hip: one FreeU site (diffusers apply_freeu) in one launch.  hidden NHWC (row stride ld_h): channels [0, C_h / 2) become
// fp16(float(x) * b) in place, everything else of a row keeps its bits.  skip NHWC (ld_s) -> skip_out NHWC (ld_d, == skip allowed): per
// (sample, channel) plane x + (s - 1) lp, lp the part of x at the frequencies {0, -1} x {0, -1} (fourier_filter with threshold 1), fp32 sums
// in a fixed order, one rounding; bytes outside [0, C_s) of a row are not written.  Either half may be null (then only the other runs).
// Any H, W >= 1.  -1: nothing to do / a size < 1; -2: C_h % 16 or C_s % 8; -3: a row stride below C, not a multiple of 8, or a pointer
// that is not 16-byte aligned.  Nothing is launched on a refusal
int ladi_launch_freeu(h16* hidden, int ld_h, int C_h, float b, const h16* skip, int ld_s, int C_s, float s, h16* skip_out, int ld_d, int n,
                      int H, int W, hipStream_t st);

// ---- pag.hip: the identity attention map of perturbed-attention guidance, O = V.  Copies rows x C halves from v (row stride ldv: the V third
// of a fused QKV buffer) to o (row stride ldo) in 16-byte vectors; columns [C, ld) of either side are never touched.  -1: a null pointer or
// rows < 1; -2: C < 8 or C % 8; -3: a row stride below C or not a multiple of 8, or a base that is not 16-byte aligned.  Nothing is launched
// on a refusal
int ladi_launch_pag_identity(const h16* v, int ldv, h16* o, int ldo, long long rows, int C, hipStream_t st);

// ---- sag.hip: self-attention guidance (StableDiffusionSAGPipeline).
// sag_map: q, k fp16 in the layout flash_attn64 reads (sample s, token t, head h at base + s * sq + t * ldq + h * 64; strides in halves,
// multiples of 8, bases 16-byte aligned), head dimension 64, any T >= 1 and any head count.  Writes s_out fp32 [n][T],
// s[j] = (sum_h sum_i softmax_j(q_i . k_j / 8)) / heads, and m_out [n][T] bytes, m = s > 1.  partial: scratch of ladi_sag_partial_floats(n, T,
// heads) floats.  fp32 accumulation, two launches, fixed-order sums: bit-reproducible.  -1: null / empty; -3: strides or alignment
long long ladi_sag_partial_floats(int n, int T, int heads);
int ladi_launch_sag_map(const h16* q, int ldq, long long sq, const h16* k, int ldk, long long sk, int n, int T, int heads, float* partial,
                        float* s_out, unsigned char* m_out, hipStream_t st);
// sag_degrade: latents fp32 [B][h * w][4] (the loop's), eps the base prediction's rows fp16 [B][h * w][ld_eps] (channels 0..3), mask bytes
// [B][hm][wm] (sag_map's m of the same samples), tab device fp32 [evals][4] = {sqrt(a), sqrt(1 - a), model-input scale, 0} read at row
// *step_idx (null: row 0).  Writes fp16(in_scale * xd) to channels 0..3 of dst_rows [B][h * w][ld_in], xd = sqrt(a) x0d + sqrt(1 - a) b,
// x0 = (x - sqrt(1 - a) b) / sqrt(a), x0d = blur9(x0) where the nearest-upsampled mask is 1 (9 x 9, sigma 1, reflect padding 4) and x0
// elsewhere.  src_rows non-null and != dst_rows: channels [4, copy_end) of src_rows are copied to dst_rows too (copy_end a multiple of 4,
// <= ld_in); otherwise nothing but channels 0..3 is written.  -2: a latent side under 5; -3: strides or alignment
int ladi_launch_sag_degrade(const float* latents, const h16* eps, int ld_eps, const unsigned char* mask, int B, int h, int w, int hm, int wm,
                            const float* tab, const int* step_idx, const h16* src_rows, h16* dst_rows, int ld_in, int copy_end, hipStream_t st);

// ---- ip_adapter.hip: the image-prompt term of a cross-attention (IP-Adapter), accumulated in place into the attention output:
//   o[s][t][h*64 + d] = fp16(float(o[..]) + scale * sum_j softmax_j(0.125 <q[s][t][h*64 ..], k[s][j][h*64 ..]>) v[s][j][h*64 + d]),  j < N
// fp32 with the row maximum subtracted, one rounding per element.  q / o: row strides ldq / ldo, per-sample strides sq / so; k / v: N rows
// per sample (strides ldk / ldv, sk / sv; the kv_cache layout is k = kv, v = kv + C, ld 2C).  Only rows t < T and columns < heads * 64 of o
// are written.  -1 (nothing launched): a null pointer, n / heads / T < 1, N outside [1, 64], ldq / ldk / ldv / ldo not a multiple of 8 or
// below heads * 64, a per-sample stride that is not a multiple of 8, a base that is not 16-byte aligned
int ladi_launch_ip_attn_add(const h16* q, int ldq, long long sq, const h16* k, int ldk, long long sk, const h16* v, int ldv, long long sv,
                            h16* o, int ldo, long long so, int n, int heads, int T, int N, float scale, hipStream_t st);
// o[row][0:C] = fp16(float(o) + scale * float(x)) over `rows` rows: the second half of the image term by the route that existed before the
// kernel above (flash_attn64 over the N keys into a scratch tensor, then this), kept as the measured A/B arm (UNet::ip_route).  C and both
// strides multiples of 8, bases 16-byte aligned, else -1
int ladi_launch_ip_scaled_add(const h16* x, int ldx, h16* o, int ldo, long long rows, int C, float scale, hipStream_t st);

// ---- tome.hip: token merging (ToMe).  Tables: src_pos[Ns] / dst_pos[Nd], token positions in ascending order (ladi_tome_tables_host, which
// returns Nd; both pointers null: only the count; -1: a size < 1, sx / sy other than 2 or cap too small).  Panels: fp16 src [n][pad_src(Ns)][C]
// and dst [n][pad_dst(Nd)][C], normalised rows, zero rows behind Ns / Nd.  Plan buffer: plan_ints(Ns, Nd, r) ints per sample,
// [seg_off (Nd + 1) | unm_pos (Ns - r) | seg_src (r) | scratch (r)] (positions are token positions, seg_off offsets into seg_src).
// Refusals (nothing launched): -1 a null pointer or a bad count (Ns + Nd != T, r outside [1, Ns] -- merge accepts r = 0 --, n > 65535 where
// n is a grid dimension); -2 the channel count (prep / match: C % 64, C <= 960; merge / unmerge: C % 8); -3 a row stride below C or not a
// multiple of 8, a per-sample stride that is not a multiple of 8, a base that is not 16-byte aligned; -4 plan: Nd > 4096
int ladi_tome_tables_host(int h, int w, int sx, int sy, int use_rand, unsigned seed, int* src_pos, int* dst_pos, int cap);
int ladi_tome_count_host(int T, int Ns, double ratio);      // r = min(int(T * ratio), Ns); -1: ratio outside [0, 1) or not finite
int ladi_tome_pad_src(int Ns);
int ladi_tome_pad_dst(int Nd);
long long ladi_tome_plan_ints(int Ns, int Nd, int r);
// x: the metric, [n][T] rows of C halves (row stride ld, per-sample stride sx)
int ladi_launch_tome_prep(const h16* x, int ld, long long sx, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int C,
                          h16* A, h16* B, hipStream_t st);
// score[n][Ns] = max_j <a_i, b_j> (fp32 accumulation on MFMA), node[n][Ns] = the lowest j that reaches it
int ladi_launch_tome_match(const h16* A, const h16* B, int n, int Ns, int Nd, int C, float* score, int* node, hipStream_t st);
// the r src with the largest score (ties to the lower src, NaN as -inf) are merged into dst node[i]: out_row[n][T] and the plan buffer
int ladi_launch_tome_plan(const float* score, const int* node, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int r,
                          int* out_row, int* plan, hipStream_t st);
// y[n][T - r]: unmerged src rows (copies), then (x[dst_j] + sum of its merged src in ascending order) / (1 + count), fp32, one rounding
int ladi_launch_tome_merge(const h16* x, int ldx, long long sx, const int* dst_pos, const int* plan, int n, int T, int Ns, int Nd, int r, int C,
                           h16* y, int ldy, long long sy, hipStream_t st);
// out[s][p] = fp16(float(y[s][out_row[s][p]]) + float(res[s][p])); an out_row entry outside [0, Tm) leaves its row unwritten
int ladi_launch_tome_unmerge_add(const h16* y, int ldy, long long sy, const h16* res, int ldr, long long sr, const int* out_row, int n, int T,
                                 int Tm, int C, h16* out, int ldo, long long so, hipStream_t st);

// ---- lora.hip: LoRA merge of one block of rows of one packed weight, from the pristine copy `base` into the live weight `W` (both fp16
// [rows of the weight][taps][cin_pad], row pitch `pitch` halves):
//   W[map(o)][t][i] = fp16(float(base[map(o)][t][i]) + sum_a scale[a] * sum_r up[a][o][r] * down[a][r][t][i]),  o < rows, i < cin
// map(o) = row0 + o, or with geglu_half = rows / 2 the GEGLU interleave of load_geglu (row0 then a multiple of 64).  up[a] fp32 [rows][rank[a]],
// down[a] fp32 [rank[a]][taps][cin].  fp32 throughout: the inner sum over ascending r, the adapters in call order, one add, one rounding; a
// delta of exactly zero keeps the base's bits, so n_adapters = 0 copies the block.  Columns [cin, cin_pad) and every other row keep their
// bits.  nonfinite (optional): += the number of results that are not finite after rounding.
// -1: null or identical base / W; -2: a size < 1, cin_pad < cin or not a multiple of 64; -3: pitch below taps * cin_pad or not a multiple of
// 8, or a base that is not 16-byte aligned; -4: a GEGLU map whose half is no multiple of 32, rows != 2 half or row0 % 64; -5: more than
// LORA_MAX_ADAPTERS; -6: a null factor or a rank outside [1, LORA_MAX_RANK]; -7: grid too large.  Nothing is launched on a refusal
enum { LORA_MAX_ADAPTERS = 8, LORA_MAX_RANK = 256 };
struct LoraMergeArgs {
    const h16* base; h16* W; long long pitch;
    int cin, cin_pad, taps;
    int row0, rows, geglu_half;
    int n_adapters;
    const float* up[LORA_MAX_ADAPTERS]; const float* down[LORA_MAX_ADAPTERS];
    int rank[LORA_MAX_ADAPTERS]; float scale[LORA_MAX_ADAPTERS];
    unsigned* nonfinite;
};
int ladi_launch_lora_merge(const LoraMergeArgs& a, hipStream_t st);

// ---- f32path.hip: fp32 kernels of the warping module (fp32 NHWC activations, fp32 weights, v_mfma_f32_32x32x2_f32)
struct ConvF32Args {
    const float* src0; const float* src1;   // up to two NHWC fp32 sources concatenated along channels
    int C0, C1, ld0, ld1;                   // channels (multiples of 8) and row strides (multiples of 4) of each source
    int Hs, Ws, Ho, Wo, P;                  // source / output spatial size per sample, output pixels = n * Ho * Wo
    int ksize, stride, pad;
    const float* W; int Q, K, ldw;          // [Q][ksize*ksize*(C0+C1)] tap-major / channel-minor (ldw = 0 -> K)
    long long bs_src0, bs_w, bs_out;        // batching over grid.z (element strides)
    const float* bias; int act;             // fp32 bias [Q] or null; LADI_ACT_NONE / RELU / TANH / SILU
    float* out; int ldo;
};
int ladi_launch_conv_f32(const ConvF32Args& a, int batch, hipStream_t st);
int ladi_launch_nchw_to_nhwc_f32(const void* src, int in_f32, int n, int C, int H, int W, float* dst, int ld, hipStream_t st);
int ladi_launch_nhwc_to_nchw_f32(const float* src, int ld, int n, int C, int H, int W, void* dst, int out_f32, hipStream_t st);
int ladi_launch_channel_affine_f32(float* x, int ld, size_t n_pix, int C, const float* scale, const float* shift, hipStream_t st);
int ladi_launch_l2norm_rows_f32(float* x, int ld, int rows, int C, hipStream_t st);
int ladi_launch_gather_rows_f32(const float* src, const int* rows, int n, int H, float* dst, hipStream_t st);
int ladi_launch_maxpool2_f32(const float* src, int lds_, int n, int H, int W, int C, float* dst, int ldd, hipStream_t st);
int ladi_launch_upsample2x_bilinear_ac_f32(const float* src, int lds_, int n, int H, int W, int C, float* dst, int ldd, hipStream_t st);
int ladi_launch_linear_f32(const float* x, int ldx, const float* W, const float* b, int M, int N, int K, int act, float* out, int ldo, hipStream_t st);

// ---- probe.hip: fp16 range probe.  Over the C valid lanes of each of `rows` rows (ld >= C halves apart; lanes C..ld-1 are never read):
// *absmax_bits = max(*absmax_bits, bits of max |x| over finite x) (atomicMax on the bits of a non-negative float), *nonfinite += number of
// inf / NaN elements.  Any C, ld and 2-byte alignment (16-byte loads when C % 8 == 0, ld % 8 == 0 and p is 16-byte aligned).
// seq / first_rank (both or neither): when this launch takes *nonfinite from zero, *first_rank = ++*seq -- the rank in time at which the
// slot first held an inf / NaN among the slots sharing `seq`
int ladi_launch_absmax_probe(const h16* p, long long rows, int C, int ld, unsigned* absmax_bits, unsigned* nonfinite, hipStream_t st,
                             unsigned* seq = nullptr, unsigned* first_rank = nullptr);

// ---- igemm per-launch timing hooks (HIP events on the launch stream); see igemm.hip
void ladi_igemm_profile_enable(int on);
void ladi_igemm_autotune(int on);   // measured tile-shape selection on first use of a problem shape (default on)
void ladi_igemm_splitk_two_pass(int on);   // 1: split-K launches use the separate reduce pass (A/B switch; default: in-launch combine)
int ladi_igemm_tuned_count();
int ladi_igemm_num_cfgs();
// {kernel family, tile_map, split factor, blocks} of the last implicit-GEMM launch (igemm_common.h ladi_igemm_note_launch)
void ladi_igemm_last_launch_info(int out[4]);
const char* ladi_igemm_cfg_symbol(int cfg);
// host-only introspection of the tile selection path (igemm.hip; none launches anything): the tune key ladi_launch_igemm would use (or its
// argument refusal code), the selection table (shipped rows + LADI_TUNE_CACHE + process-local puts; cfg 0 erases, returns the previous value),
// cfg_admissible itself, {cfg, source} of the last top-level launch (0 explicit, 1 table, 2 measured now, 3 cost model, 4 gn_ss list), and the
// text log of distinct top-level launches
int ladi_igemm_key_of(const IGemmArgs& a, int batch, int key[8]);
int ladi_igemm_tuned_lookup(const int key[8]);
int ladi_igemm_tuned_put(const int key[8], int cfg);
int ladi_igemm_admissible(const IGemmArgs& a, int batch, int cfg, int strict);
void ladi_igemm_selection(int out[2]);
void ladi_igemm_log_enable(int on);
int ladi_igemm_log_read(char* buf, int n);
int ladi_igemm_profile_collect(double* out, int n_out);
// the same records grouped by kernel SYMBOL (exact rocprofv3 name): lines "symbol\tms\tflop\tlaunches\n" into buf (truncated at n); does
// NOT clear the records (call before ladi_igemm_profile_collect)
int ladi_igemm_profile_symbols(char* buf, int n);
