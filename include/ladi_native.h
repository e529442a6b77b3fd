/*
 * libladi_native — C ABI of the MI355X-native LaDI-VTON denoising hot path.
 *
 * The reference (miccunifi/ladi-vton) has no FFI / operator registry: its seam is the Python nn.Module duck type that
 * StableDiffusionTryOnePipeline is constructed from (src/vto_pipelines/tryon_pipe.py:56-68,129-137; built at
 * src/inference.py:212-220).  Each group of entry points below replaces exactly one of those modules; the citation
 * next to it is the reference interface it stands in for.  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - Every function returns 0 on success and a negative code on failure; ladi_last_error() returns a message
 *     (thread local).  Nothing throws across the boundary.
 *   - Pointers named *_dev are DEVICE pointers owned by the caller (e.g. torch allocations); the library never frees
 *     them.  `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).  All work is
 *     enqueued asynchronously on that stream; no entry point synchronises except where stated.
 *   - dtype codes: 0 = float32, 1 = float16.
 *   - Handles are not thread-safe (one pipeline per process per GPU, as in the reference).
 *   - The library has NO CPU fallback: without a gfx950 device every compute entry point fails.
 */
#ifndef LADI_NATIVE_H
#define LADI_NATIVE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LADI_F32 0
#define LADI_F16 1

const char* ladi_last_error(void);
int ladi_version(void);
/* number of visible HIP devices (0 when there is no GPU); never fails */
int ladi_device_count(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Weight store: host-side staging of a diffusers-format state_dict (replaces nn.Module.load_state_dict,
 * hubconf.py:28,39,55; key names per SURVEY.md App. A.6).  Data is copied; the caller may free its buffer.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct ladi_weights ladi_weights;
ladi_weights* ladi_weights_create(void);
int ladi_weights_add(ladi_weights* ws, const char* key, const void* host_data, int dtype, int ndim, const int64_t* shape);
int ladi_weights_count(const ladi_weights* ws);
void ladi_weights_destroy(ladi_weights* ws);

/* ---------------------------------------------------------------------------------------------------------------
 * UNet — replaces diffusers UNet2DConditionModel as built by hubconf.py:31-39 (in_channels = 31) and called at
 * tryon_pipe.py:732: unet(latent_model_input, t, encoder_hidden_states=prompt_embeds).sample
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int in_channels, out_channels;
    int block_out_channels[4];
    int num_heads[4];            /* diffusers "attention_head_dim" used as head COUNT; head dim must be 64 */
    int layers_per_block;
    int cross_attention_dim;
    int norm_num_groups;
    float norm_eps;
} ladi_unet_config;
typedef struct ladi_unet ladi_unet;
ladi_unet* ladi_unet_create(const ladi_unet_config* cfg, const ladi_weights* ws);
void ladi_unet_destroy(ladi_unet* u);
/* encoder_hidden_states [n, L, cross_attention_dim] fp16 dense; precomputes the cross-attention K/V of all blocks */
int ladi_unet_set_context(ladi_unet* u, const void* ehs_dev, int n, int L, void* stream);
/* sample [n, in_channels, h, w] NCHW (dtype), scalar timestep, out [n, out_channels, h, w] NCHW (out_dtype).
 * Size contract: any h, w (images of any side divisible by 8; the tests run latents from 3x3 to 128x96).  As diffusers' UNet2DConditionModel: the stride-2 downsamplers give
 * ceil(side / 2), and when h or w is not a multiple of 8 every upsampler stretches to the size of the skip it is concatenated with
 * (`forward_upsample_size`, nearest as F.interpolate(size=...)); multiples of 8 double at every level, as before. */
int ladi_unet_forward(ladi_unet* u, const void* sample_dev, int dtype, int n, int h, int w, float timestep, void* out_dev,
                      int out_dtype, void* stream);
/* ladi_unet_forward with the deep-feature cache of the first (full-resolution) level (DeepCache; layer names are diffusers', L =
 * layers_per_block).  The cached tensor is the hidden state that enters up_blocks.3.resnets.(L - branch), before the concatenation with its
 * skip: the output of up_blocks.3.attentions.(L - branch - 1), or of up_blocks.2.upsamplers.0 for branch = L.  It is fp16 [n, h, w, C] with C =
 * block_out_channels[0] (branch < L) or block_out_channels[1] (branch = L), owned by the handle, one row per sample of the context batch.
 *   mode 0: ladi_unet_forward.
 *   mode 1: the whole forward (same launches, same result), which also copies that tensor into the cache.
 *   mode 2: the shallow forward from the cache: conv_in, layers 0 .. branch-1 of down_blocks.0 (resnet + attention), then up_blocks.3 layers
 *           L-branch .. L, each with its usual skip, the first taking the cached tensor as its hidden state, conv_norm_out, conv_out; the time
 *           embedding is that of `timestep`.  Nothing of the deeper levels or the mid block runs.
 * branch: 0 .. L.  Mode 2 without a capture at the same (n, h, w, branch) since the last ladi_unet_set_context is an error with a message;
 * nothing is launched.  A set_context, or a capture at another (h, w, branch), drops what the cache held. */
int ladi_unet_forward_cached(ladi_unet* u, const void* sample_dev, int dtype, int n, int h, int w, float timestep, void* out_dev,
                             int out_dtype, int mode, int branch, void* stream);
/* Supported ABI, beyond the single-call form above (which is this entry with sample0 = 0 and n = the context's n): the same over n samples
 * that start at index sample0 of the context batch (sample0 + n <= the context's n).  They use their own rows of the cross-attention K/V
 * and of the feature cache, as a cond-only evaluation of the fused loop does (NativeUNet's `sample0=`; with mode 0 it is the plain forward
 * over those rows).  Mode 2 needs every one of these rows captured (by whichever calls) at the same (h, w, branch). */
int ladi_unet_forward_cached_rows(ladi_unet* u, const void* sample_dev, int dtype, int n, int h, int w, float timestep, void* out_dev,
                                  int out_dtype, int mode, int branch, int sample0, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * VAE — replaces src/models/AutoencoderKL.py AutoencoderKL.encode (:145-157) / .decode (:174-188) with the EMASC
 * wiring of src/models/vae.py Encoder.forward (:99-119) / Decoder.forward (:183-212).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int in_channels, out_channels, latent_channels;
    int block_out_channels[4];
    int layers_per_block;
    int norm_num_groups;
    float scaling_factor;
} ladi_vae_config;
typedef struct ladi_vae ladi_vae;
ladi_vae* ladi_vae_create(const ladi_vae_config* cfg, const ladi_weights* ws);
void ladi_vae_destroy(ladi_vae* v);
/* x [B,3,H,W] NCHW (dtype) -> moments [B, 2*latent, H/8, W/8] NCHW fp32 (quant_conv applied) and, when feats_dev is
 * non-NULL, the five intermediate features idx1..5 written NHWC fp16 into caller buffers
 * ([B,H,W,c0] [B,H,W,c0] [B,H/2,W/2,c0] [B,H/4,W/4,c1] [B,H/8,W/8,c2], c = block_out_channels). */
int ladi_vae_encode(ladi_vae* v, const void* x_dev, int dtype, int B, int H, int W, float* moments_dev, void* const* feats_dev,
                    void* stream);
/* z [B,latent,h,w] NCHW fp32 (already divided by scaling_factor, as vae.decode receives it), skips_dev = NULL or five
 * NHWC fp16 EMASC outputs (idx1..5 order) -> sample [B,3,8h,8w] NCHW (out_dtype), NOT post-processed. */
int ladi_vae_decode(ladi_vae* v, const float* z_dev, int B, int h, int w, const void* const* skips_dev, void* sample_dev,
                    int out_dtype, void* stream);
/* fp16-range guard of the decoder (SD VAE activations can leave the fp16 range with real checkpoints; the reference
 * runs src/models/AutoencoderKL.py:159-188 in whatever dtype the caller picked).  The decoder's residual stream is stored multiplied by
 * 2^-shift (GroupNorm is scale invariant, every branch into the stream is scaled in its producer's epilogue): the same function with
 * 2^shift more head-room.  shift = -1 (default): automatic -- decode at shift 0 and, if a GroupNorm saw non-finite statistics, again at 4,
 * then 8 (an error after that); shift >= 0: fixed.  ladi_vae_last_range_shift reports what the last decode used. */
int ladi_vae_set_range_shift(ladi_vae* v, int shift);
int ladi_vae_last_range_shift(const ladi_vae* v);

/* ---------------------------------------------------------------------------------------------------------------
 * EMASC — replaces src/models/emasc.py EMASC.forward (:37-40); mask_features (src/utils/data_utils.py:4-16) can be
 * fused by passing the binarised full-resolution mask.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int n; int in_channels[8]; int out_channels[8]; } ladi_emasc_config;
typedef struct ladi_emasc ladi_emasc;
ladi_emasc* ladi_emasc_create(const ladi_emasc_config* cfg, const ladi_weights* ws);
void ladi_emasc_destroy(ladi_emasc* e);
/* feats_dev[i]: NHWC fp16 [B, hs[i], wss[i], in_channels[i]] ; outs_dev[i]: NHWC fp16 [B, hs[i], wss[i], out_channels[i]].
 * mask_dev: NULL, or [B, Hm, Wm] fp16 binary mask at full resolution (Hm = hs[0]): out *= (1 - nearest(mask)). */
int ladi_emasc_forward(ladi_emasc* e, const void* const* feats_dev, const int* hs, const int* wss, int B, const void* mask_dev,
                       int Hm, int Wm, void* const* outs_dev, void* stream);
/* stand-alone mask_features on one NHWC fp16 feature map (in place): feat *= (1 - nearest(mask -> h x w)) */
int ladi_mask_features(void* feat_dev, int B, int h, int w, int C, const void* mask_dev, int Hm, int Wm, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Inversion adapter — replaces src/models/inversion_adapter.py InversionAdapter.forward (:22-28), dims hubconf.py:17-24
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int hidden, heads, mlp_dim, head_hidden, out_dim; float layer_norm_eps; } ladi_adapter_config;
typedef struct ladi_adapter ladi_adapter;
ladi_adapter* ladi_adapter_create(const ladi_adapter_config* cfg, const ladi_weights* ws);
void ladi_adapter_destroy(ladi_adapter* a);
/* x [B, T, hidden] fp16 dense -> out [B, out_dim] fp16 */
int ladi_adapter_forward(ladi_adapter* a, const void* x_dev, int B, int T, void* out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * CLIP text encoder with pseudo-word splice — replaces src/utils/encode_text_word_embedding.py encode_text_word_embedding
 * (:6-72; call site src/inference.py:291-295) and the transformers CLIPTextModel it drives (SD2 text encoder: 23 layers, 1024-d,
 * 16 heads, gelu MLP 4096, 77 positions, causal).  SURVEY.md §8(f) rank 1: the producer of `prompt_embeds`.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int vocab_size, hidden, heads, mlp_dim, layers, max_positions, vstar_token_id; float layer_norm_eps; } ladi_text_config;
typedef struct ladi_text_encoder ladi_text_encoder;
/* weights: transformers-4.27 key layout (text_model.embeddings.*, text_model.encoder.layers.N.*, text_model.final_layer_norm.*);
 * the flattened layout without the text_model. prefix is accepted too */
ladi_text_encoder* ladi_text_encoder_create(const ladi_text_config* cfg, const ladi_weights* ws);
void ladi_text_encoder_destroy(ladi_text_encoder* t);
/* input_ids_host: [B][T] int32 in HOST memory (tokenizer output); word_embeddings_dev: fp16 [B][num_vstar][hidden] or NULL (no splice).
 * In every sentence containing vstar_token_id ('$' = 259) the num_vstar positions starting at its FIRST occurrence are replaced by that
 * sentence's pseudo-word embeddings (:12-35); slots running past T are an error (the reference raises IndexError).
 * out_hidden_dev: fp16 [B][T][hidden] = final_layer_norm(encoder output) (:56-57); out_pooled_dev: fp16 [B][hidden] = row at
 * argmax(input_ids) (:62-65), or NULL. */
int ladi_text_encoder_forward(ladi_text_encoder* t, const int* input_ids_host, int B, int T, const void* word_embeddings_dev,
                              int num_vstar, void* out_hidden_dev, void* out_pooled_dev, void* stream);
/* the same with input_ids already in DEVICE memory (the reference moves them there before the call, src/inference.py:291): the first '$'
 * and the end-of-text row are found by a kernel and nothing crosses the host, so the call never synchronises.  No host-side validation in
 * this form: ids are clamped to the vocabulary by the lookup and slots running past T are cut instead of raising. */
int ladi_text_encoder_forward_dev(ladi_text_encoder* t, const int* input_ids_dev, int B, int T, const void* word_embeddings_dev,
                                  int num_vstar, void* out_hidden_dev, void* out_pooled_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * CLIP ViT-H/14 vision encoder — replaces the transformers CLIPVisionModelWithProjection forward the reference calls at
 * src/inference.py:269-273 (`vision_encoder(pixel_values).last_hidden_state`, fed to the inversion adapter at :276).
 * SURVEY.md §8(f) rank 2.  32 layers, 1280-d, 16 heads of 80, gelu MLP 5120, 224x224 / patch 14 -> 257 tokens.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int hidden, heads, mlp_dim, layers, image_size, patch_size; float layer_norm_eps; } ladi_vision_config;
typedef struct ladi_vision_encoder ladi_vision_encoder;
/* weights: transformers-4.27 key layout (vision_model.embeddings.*, vision_model.pre_layrnorm.*, vision_model.encoder.layers.N.*,
 * vision_model.post_layernorm.*); the flattened layout without the vision_model. prefix is accepted too.  visual_projection.weight
 * ([projection_dim, hidden], no bias: CLIPVisionModelWithProjection) is loaded when the weights hold it -- it only feeds
 * ladi_vision_encoder_forward_ex's image_embeds; without the key the encoder is the same in every respect */
ladi_vision_encoder* ladi_vision_encoder_create(const ladi_vision_config* cfg, const ladi_weights* ws);
void ladi_vision_encoder_destroy(ladi_vision_encoder* v);
/* pixel_values_dev: [B,3,S,S] (dtype: 0 fp32, 1 fp16), already CLIP-normalised (the CLIPProcessor stays on the caller's side);
 * out_hidden_dev: fp16 [B][1 + (S/ps)^2][hidden] = last_hidden_state (encoder output, NO post_layernorm);
 * out_pooled_dev: fp16 [B][hidden] = post_layernorm(last_hidden_state[:, 0]) (pooler_output) or NULL */
int ladi_vision_encoder_forward(ladi_vision_encoder* v, const void* pixel_values_dev, int dtype, int B, void* out_hidden_dev,
                                void* out_pooled_dev, void* stream);
/* projection_dim of the loaded visual_projection.weight, 0 when the weights held none (-1: null handle) */
int ladi_vision_encoder_projection_dim(const ladi_vision_encoder* v);
/* ladi_vision_encoder_forward with every output optional (NULL: not produced; with all four NULL nothing is launched) and two more:
 * out_penultimate_dev: fp16 [B][tokens][hidden] = the INPUT of the last encoder layer, i.e. transformers' hidden_states[-2], no
 *   post_layernorm (what the IP-Adapter Plus Resampler reads); with layers == 1 it is the pre_layrnorm output.  Its producer writes it
 *   directly, as the last layer writes out_hidden_dev.
 * out_image_embeds_dev: fp16 [B][projection_dim] = visual_projection(pooler_output).  Asking for it without a loaded projection is an
 *   error with a message, and nothing is launched or written.
 * out_hidden_dev and out_pooled_dev hold the bits ladi_vision_encoder_forward gives. */
int ladi_vision_encoder_forward_ex(ladi_vision_encoder* v, const void* pixel_values_dev, int dtype, int B, void* out_hidden_dev,
                                   void* out_pooled_dev, void* out_penultimate_dev, void* out_image_embeds_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Resampler — the image projection of IP-Adapter Plus (tencent-ailab/IP-Adapter `Resampler`, a Perceiver resampler): hidden states of
 * the image encoder [n][T][E] -> N image tokens [n][N][out_dim].  The arithmetic (csrc/runtime_resampler.cpp) is restated from memory of
 * that package, which is not a dependency, and was not checked against it.  Runs once per call, from the kernels of the hot path.
 * weights: the original key layout -- latents [1, N, dim], proj_in.{weight,bias}, proj_out.{weight,bias}, norm_out.{weight,bias} and per
 * layer i: layers.i.0.norm1.*, layers.i.0.norm2.*, layers.i.0.to_q.weight [inner, dim], layers.i.0.to_kv.weight [2 inner, dim],
 * layers.i.0.to_out.weight [dim, inner], layers.i.1.0.{weight,bias} (LayerNorm), layers.i.1.1.weight, layers.i.1.3.weight (bias-free).
 * The geometry comes from the weights; heads = inner / dim_head.  Refused at create, with a message and before the device is touched:
 * N outside 1..64, dim_head not one of 64 / 80 / 96 / 128, inner % dim_head != 0, E, dim or out_dim not a multiple of 8 (dim and
 * out_dim at most 4096), no layer, a missing, mis-shaped or unexpected key.  T is free (>= 1).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct ladi_resampler ladi_resampler;
ladi_resampler* ladi_resampler_create(const ladi_weights* ws, int dim_head);
void ladi_resampler_destroy(ladi_resampler* r);
/* any output pointer may be NULL */
int ladi_resampler_info(const ladi_resampler* r, int* N, int* E, int* dim, int* depth, int* heads, int* out_dim);
/* x_dev fp16 [n][T][E] dense -> tokens_out_dev fp16 [n][N][out_dim] dense, asynchronous on `stream` */
int ladi_resampler_forward(ladi_resampler* r, const void* x_dev, int n, int T, void* tokens_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Refinement UNet of the warping module — replaces src/models/UNet.py UNetVanilla.forward (:23-34; parts in src/models/unet_parts.py)
 * as instantiated by hubconf.py:57 (24 -> 3 channels, bilinear=True) and called at src/inference.py:264.  SURVEY.md §8(f) rank 3
 * (first half; the TPS matching network is not native yet).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int in_channels, out_channels, base_channels; float bn_eps; } ladi_refine_config;
typedef struct ladi_refine ladi_refine;
/* weights: the 'refinement' state_dict of the released warping checkpoint (hubconf.py:62): inc.double_conv.*, downN.maxpool_conv.1.*,
 * upN.conv.double_conv.*, outc.conv.*; BatchNorm running statistics are folded into the convolutions (inference mode) */
ladi_refine* ladi_refine_create(const ladi_refine_config* cfg, const ladi_weights* ws);
void ladi_refine_destroy(ladi_refine* r);
/* x_dev: [B, in_channels, H, W] NCHW (dtype 0 fp32 / 1 fp16), H and W multiples of 16; out_dev: [B, out_channels, H, W] NCHW (out_dtype) */
int ladi_refine_forward(ladi_refine* r, const void* x_dev, int dtype, int B, int H, int W, void* out_dev, int out_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * TPS geometric-matching network of the warping module — replaces the inference data flow of src/models/ConvNet_TPS.py
 * ConvNet_TPS.forward (:315-337) as instantiated by hubconf.py:56 (256x192, input_nc 21, n_layer 3) and called at
 * src/inference.py:253 (`low_grid, theta, ... = tps(low_cloth, agnostic)`).  SURVEY.md §8(f) rank 3 (second half).
 * The training-only regulariser outputs (rx, ry, cx, cy, rg, cg; :201-224) are not produced.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct { int height, width, input_nc, n_layers, grid_size, ngf; float bn_eps; } ladi_tps_config;
typedef struct ladi_tps ladi_tps;
/* weights: the 'tps' state_dict of the released warping checkpoint (hubconf.py:61); gridGen.* buffers are recomputed, not read */
ladi_tps* ladi_tps_create(const ladi_tps_config* cfg, const ladi_weights* ws);
void ladi_tps_destroy(ladi_tps* t);
/* input_a_dev [B,3,H,W], input_b_dev [B,input_nc,H,W] NCHW (dtype 0 fp32 / 1 fp16); grid_dev: fp32 [B,H,W,2] sampling grid in [-1,1]
 * (x, y) as F.grid_sample expects; coor_dev: fp32 [B, grid_size^2, 2] source control points (theta) or NULL */
int ladi_tps_forward(ladi_tps* t, const void* input_a_dev, const void* input_b_dev, int dtype, int B, float* grid_dev, float* coor_dev,
                     void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Scheduler — replaces diffusers DDIMScheduler / PNDMScheduler (skip_prk_steps) / LMSDiscreteScheduler set_timesteps +
 * scale_model_input + step (tryon_pipe.py:62,424,650-651,722,740), and the diffusers 0.14 DPMSolverMultistepScheduler
 * (algorithm_type dpmsolver++), EulerDiscreteScheduler (s_churn 0) and EulerAncestralDiscreteScheduler, all with epsilon prediction.
 * Scheduler code (the `kind` / `scheduler` argument): bits 0-3 the kind,
 *   0 = DDIM, 1 = PNDM, 2 = LMSDiscrete, 3 = DPMSolverMultistep (dpmsolver++), 4 = EulerDiscrete, 5 = EulerAncestralDiscrete;
 * bits 8-11 DPM-Solver++ options (kind 3 only; the code 3 alone is DPM-Solver++ 2M, midpoint, lower_order_final):
 *   bits 8-9 solver_order (0 = 2, or 1..3), bit 10 solver_type heun (0 = midpoint), bit 11 lower_order_final off.
 * Any other bit, an option bit on another kind or an unknown kind is an error.  The DPM / Euler formulas are restated from the published
 * algorithms as diffusers 0.14 ships them, not pinned against diffusers itself (it is not installable here).
 *
 * Few-step sampling (distilled weights: LCM / LCM-LoRA, TCD, Turbo, Lightning, Hyper-SD).  Two more kinds and two more option fields:
 *   7 = LCM, 8 = TCD (kinds 6, 9 and 15 stay unknown);
 *   bit 6 = trailing timestep spacing, valid on kinds 0 (DDIM), 4 (Euler) and 5 (Euler-ancestral) only;
 *   bits 12-21 = original_inference_steps of LCM / TCD, 1..1000 (0 = 50), valid on kinds 7 and 8 only.
 * num_inference_steps N: [1, original_inference_steps] for kinds 7 and 8, [1, 1000] with the trailing bit, [2, 1000] for the plain codes 0-5.
 * The arithmetic below is restated from the published algorithms as diffusers ships them, from memory like the other schedulers here; THIS
 * TEXT IS THE CONTRACT.  a(t) = alphas_cumprod[t], T = 1000, every coefficient is computed in double and the rows are held in fp32; the
 * timesteps of the evaluations i = 0..N-1:
 *   LCM / TCD : O = original_inference_steps, k = T / O (integer division), t_i = (O - floor(i * (O / N))) * k - 1 with i * (O / N) evaluated
 *               in double as numpy.linspace(0, O, N, endpoint=False) evaluates it (O = 50: N = 4 gives 999, 759, 499, 259; N = 1 gives 999).
 *   trailing  : t_i = round_half_even(T - i * (T / N)) - 1 (N = 4: 999, 749, 499, 249; N = 3: 999, 666, 332).  This closed form is the
 *               contract.  It equals np.round(np.arange(T, 0, -T/N)) - 1 for every N <= 47; from N = 48 on, numpy's arange sometimes
 *               differs in a value or returns one element too many.  It gives no duplicate and no negative timestep for any N in 1..1000.
 * With x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t), the updates, all linear in (x, eps, noise_i) and therefore rows of the table below:
 *   LCM       : s = 10 t (timestep_scaling 10, sigma_data 0.5), c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25),
 *               den = c_out x0 + c_skip x; x' = sqrt(a_p) den + sqrt(1 - a_p) noise_i with a_p = a(t_{i+1}); the last evaluation x' = den
 *               (c_n = 0).  Row: c_x = sqrt(a_p) (c_out / sqrt(a_t) + c_skip), c_e w0 = -sqrt(a_p) c_out sqrt(1 - a_t) / sqrt(a_t),
 *               c_n = sqrt(1 - a_p), sqrt(a_p) replaced by 1 in the last row.
 *   TCD       : gamma = eta in [0, 1]; t_prev = t_{i+1}, or 0 after the last timestep; t_s = floor((1 - gamma) t_prev);
 *               x_s = sqrt(a_s) x0 + sqrt(1 - a_s) eps; gamma > 0 and not the last evaluation: x' = sqrt(a_prev / a_s) x_s +
 *               sqrt(1 - a_prev / a_s) noise_i; otherwise x' = x_s.  gamma = 0 is the deterministic DDIM jump t_i -> t_{i+1}, the last to t = 0.
 *   trailing DDIM : DDIM's row (with or without eta) over the trailing timesteps with diffusers' prev = t - T / N (integer division; N = 3:
 *               666, 333, -1, not the next timestep); prev < 0 uses alphas_cumprod[0].
 *   trailing Euler / Euler-ancestral : their rows over sigma_i = sqrt((1 - a(t_i)) / a(t_i)) held in fp32, with a trailing 0;
 *               init_noise_sigma is the largest sigma (14.6146 at t = 999 with the default betas); a one-step Euler-ancestral row has
 *               sigma_up = 0.
 * The rules generic over kinds cover kinds 7 and 8 like DDIM: a tail (first_step, strength) is the tail of the N-step list and starts from
 * sqrt(a) init + sqrt(1 - a) noise at its first timestep (not diffusers' set_timesteps(strength=)); the latent blend's coefficients are
 * sqrt(a), sqrt(1 - a) at timesteps[i + 1]; the cloth cut-off counts evaluations.  Step noise: a run whose table has a stochastic term needs
 * one slab per evaluation; LCM, and TCD with eta > 0, never read the last slab (its row has c_n = 0), and a run of one evaluation needs none.
 * Not covered: guidance-embedded UNets (time_cond_proj_dim / timestep_cond), trailing spacing on PNDM, LMS and DPM-Solver++,
 * timestep_scaling != 10, v-prediction, custom timestep lists.
 * ------------------------------------------------------------------------------------------------------------- */
#define LADI_SCHED_DDIM 0
#define LADI_SCHED_PNDM 1
#define LADI_SCHED_LMS 2
#define LADI_SCHED_DPMPP 3
#define LADI_SCHED_EULER 4
#define LADI_SCHED_EULER_ANCESTRAL 5
#define LADI_SCHED_LCM 7
#define LADI_SCHED_TCD 8
#define LADI_SCHED_TRAILING (1 << 6)           /* kinds 0, 4 and 5 */
#define LADI_SCHED_ORIGINAL_STEPS(o) ((o) << 12)     /* kinds 7 and 8; o in 1..1000, 0 = 50 */
#define LADI_SCHED_DPM_ORDER(o) ((o) << 8)     /* o in 1..3 */
#define LADI_SCHED_DPM_HEUN (1 << 10)
#define LADI_SCHED_DPM_NO_LOWER_ORDER_FINAL (1 << 11)
/* host helper: writes the N (DDIM, DPMSolverMultistep, LCM, TCD, any trailing code) or N+1 (PNDM) integer timesteps; returns their count,
 * or negative on error.  LMSDiscrete / Euler / Euler-ancestral without the trailing bit (fractional timesteps) are refused: use
 * ladi_sched_lms, whose timesteps and sigmas all three share.
 * DPMSolverMultistep refuses step counts whose rounded timesteps repeat (N = 1000), on which diffusers 0.14 fails. */
int ladi_sched_timesteps(int kind, int num_inference_steps, int* timesteps_out, int cap);
/* host helper (tests): the per-evaluation step table of any scheduler code, 10 floats per evaluation:
 *   [c_x, c_e, w0, w1, w2, w3, p_x, p_e, c_n, in_scale_next]:  x' = c_x x + c_e sum_k w_k h_k + c_n noise, where h_0 is the guided eps
 *   (DDIM / PNDM / LMS / Euler) or the data prediction p_x x + p_e eps (DPMSolverMultistep), and h_k (k > 0) the earlier ones;
 *   in_scale_next = scale_model_input of the next evaluation.  timesteps_out[evals] (float64) and rows_out may be null.
 * Returns the evaluation count (or negative on error; cap = capacity in evaluations). */
int ladi_sched_table(int kind, int num_inference_steps, const float* alphas_cumprod_host, double* timesteps_out, float* rows_out, int cap);
/* the same table for DDIMScheduler.step(eta = ...) (diffusers 0.14): std = eta sqrt(max((1 - a_p) / (1 - a_t) (1 - a_t / a_p), 0)), the eps
 * direction sqrt(max(1 - a_p - std^2, 0)), c_n = std.  eta == 0 gives ladi_sched_table's rows bit for bit.  TCD's gamma travels as eta too
 * (diffusers' TCDScheduler.step takes it under that name) and has to be in [0, 1].  eta < 0, a non-finite eta, or a non-zero eta with any
 * kind but DDIM and TCD is an error (the other schedulers' step() takes no eta). */
int ladi_sched_table_eta(int kind, int num_inference_steps, const float* alphas_cumprod_host, float eta, double* timesteps_out, float* rows_out,
                         int cap);
/* the table of a run that starts at step first_step of the num_inference_steps-step schedule (strength; ladi_tryon_set_init): the evaluations of
 * steps first_step .. with the timesteps and sigmas of those steps, indexed from 0, same row layout.  Multistep history starts empty at the new
 * start: LMSDiscrete and DPMSolverMultistep warm up again (orders 1, 2, ..), lower_order_final acts where it does in the whole run.  PNDM
 * restarts as a fresh PLMS run over the tail's step timesteps u0 > u1 > ..: evaluations [u0, u1, u1, u2, ..], one more than tail steps -- NOT
 * diffusers' slice of the N + 1 list, which leaves the sample one step under-denoised; a PNDM tail needs 2 steps (first_step <= N - 2), the
 * others 1 (first_step <= N - 1).  start_out (may be null) = {k_x, k_n, in_scale0}: the start latents are k_x * init + k_n * noise (DDIM / PNDM /
 * DPMSolverMultistep: sqrt(a_t), sqrt(1 - a_t) at t = timesteps[first_step]; LMS / Euler / Euler-ancestral: 1, sigma[first_step]; computed in
 * double), in_scale0 the scale_model_input of the first evaluation.  first_step = 0 gives ladi_sched_table_eta's rows and timesteps bit for bit
 * and start_out = {0, init_noise_sigma, in_scale0}.  A first_step out of range is an error. */
int ladi_sched_table_from(int kind, int num_inference_steps, const float* alphas_cumprod_host, float eta, int first_step, double* timesteps_out,
                          float* rows_out, int cap, float* start_out);
/* host helper, LMSDiscrete (order 4): timesteps_out[N] (fractional, float64 as diffusers holds them), sigmas_out[N + 1] (trailing 0;
 * init_noise_sigma = sigmas_out[0]), coeffs_out[N][4] = linear-multistep weights of evaluation i over its derivatives
 * [d_i, d_{i-1}, d_{i-2}, d_{i-3}] (zero beyond the order min(i + 1, 4)).  alphas_cumprod_host null = default.  Any output may be null. */
int ladi_sched_lms(int num_inference_steps, const float* alphas_cumprod_host, double* timesteps_out, float* sigmas_out, float* coeffs_out);
/* host helper: default alphas_cumprod (scaled_linear 0.00085..0.012, 1000 steps), out[1000] */
/* coefficients of the latent blend (ladi_tryon_set_preserve) of a run that starts at step first_step: out[i] = {k_x, k_n} of the scheduler's
 * add_noise at timesteps[i + 1] (DDIM / PNDM / DPM-Solver++: sqrt(a), sqrt(1 - a); LMS / Euler / Euler-ancestral: 1, sigma[i + 1]), computed in
 * double and held in fp32; the last row is {1, 0}.  One row per evaluation of ladi_sched_table_from; returns their count, < 0 when it exceeds cap */
int ladi_sched_keep_coeffs(int kind, int num_inference_steps, const float* alphas_cumprod_host, int first_step, float* out, int cap);
int ladi_sched_alphas_cumprod(float* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Whole-loop fast path — StableDiffusionTryOnePipeline.__call__ steps 4-11 (tryon_pipe.py:630-753) in one call.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int batch, height, width;
    int in_dtype;                      /* dtype of image / mask_image / pose_map / warped_cloth */
    const void* image_dev;             /* [B,3,H,W] in [-1,1] */
    const void* mask_image_dev;        /* [B,1,H,W] in [0,1] (binarised at 0.5 like prepare_mask_and_masked_image) */
    const void* pose_map_dev;          /* [B,P,H,W] */
    const void* warped_cloth_dev;      /* [B,3,H,W] or NULL (cloth_input_type == 'none') */
    int pose_channels;
    const void* prompt_embeds_dev;           /* [B,L,D] fp16 */
    const void* negative_prompt_embeds_dev;  /* [B,L,D] fp16 (required when guidance_scale > 1) */
    int L;
    const float* noise_cloth_dev;      /* fp32 [B,4,h,w]: the three generator draws in pipeline order */
    const float* noise_latents_dev;
    const float* noise_masked_dev;
    int num_inference_steps;
    float guidance_scale;
    int scheduler;                     /* scheduler code (see "Scheduler" above): 0 DDIM, 1 PNDM, 2 LMSDiscrete, 3 DPMSolverMultistep
                                        * (+ option bits), 4 EulerDiscrete, 5 EulerAncestralDiscrete (needs ladi_tryon_set_step_noise),
                                        * 7 LCM (step noise when it has more than one evaluation), 8 TCD (step noise with eta > 0),
                                        * + LADI_SCHED_TRAILING / LADI_SCHED_ORIGINAL_STEPS; DDIM's eta and TCD's gamma are set with
                                        * ladi_tryon_set_eta.  num_inference_steps may be 1 for kinds 7 and 8 and with the trailing bit */
    int cloth_zero_from_eval;          /* first evaluation index i that sees zero cloth latents: the smallest i with
                                        * i >= num_inference_steps - (1 - cloth_cond_rate) * num_inference_steps, evaluated by the CALLER in
                                        * float64 exactly like tryon_pipe.py:654,718 (a float32 rate crossing the ABI shifts the cut-off by
                                        * one step for rates such as 0.2 / 0.4 / 0.6 / 0.8); >= the evaluation count: never */
    int no_pose;
    int use_graph;                     /* capture the denoising step into a hipGraph and replay it */
    const float* alphas_cumprod_host;  /* optional [1000] override */
} ladi_tryon_inputs;
typedef struct ladi_tryon ladi_tryon;
/* emasc may be NULL (pipeline without EMASC); handles stay owned by the caller */
ladi_tryon* ladi_tryon_create(ladi_unet* unet, ladi_vae* vae, ladi_emasc* emasc);
void ladi_tryon_destroy(ladi_tryon* t);
/* images_dev: fp32 [B,H,W,3] in [0,1] (decode_latents layout, tryon_pipe.py:356-358); latents_dev: optional fp32 [B,4,h,w].
 * H and W: any multiple of 8 (ladi_unet_forward's size contract for the latent h = H / 8, w = W / 8). */
int ladi_tryon_run(ladi_tryon* t, const ladi_tryon_inputs* in, float* images_dev, float* latents_dev, void* stream);
/* the same call with the batch in the dtype numpy_to_pil produces (tryon_pipe.py:357-360): uint8 [B,H,W,3] = round(image * 255),
 * round-half-to-even like numpy -- what the RCCL all-gather of the sharded path and the JPEG encoder consume */
int ladi_tryon_run_u8(ladi_tryon* t, const ladi_tryon_inputs* in, unsigned char* images_dev, float* latents_dev, void* stream);
/* per-evaluation trace for parity tests (tryon_pipe.py:732-740 intermediate values): subsequent runs write the guided noise prediction
 * and the updated latents of evaluation i to *_trace_dev[i] (fp32 [B, h*w, 4] each) for i < cap_evals; NULL pointers switch it off.
 * Buffers are caller-owned and must outlive the runs. */
int ladi_tryon_set_trace(ladi_tryon* t, float* eps_trace_dev, float* latents_trace_dev, int cap_evals);
/* per-step noise of EulerAncestralDiscrete, of DDIM with eta > 0, of LCM and of TCD with eta > 0 (the randn draw of their step(), one slab
 * per evaluation; LCM and TCD draw at every evaluation but the last, whose slab is never read and may hold anything): fp32
 * [steps][B][4][h][w] on the device.  Each run copies the first `evaluations` steps on its stream into a runtime-owned buffer before the loop,
 * so the captured graph never reads the caller's buffer (which, like the run's other inputs, must stay valid until the run's work on the stream
 * has started); such a run with no noise, or fewer steps than evaluations, fails.  Runs without a stochastic term ignore it.  NULL = off. */
int ladi_tryon_set_step_noise(ladi_tryon* t, const float* noise_dev, int steps);
/* start the following runs from given latents at step first_step of the schedule instead of from noise at step 0 (strength; sticky per handle):
 * init_latents_dev fp32 [B][4][hs][ws] on the device, in the loop's latent space (x scaling_factor), e.g. the latents_dev of an earlier run.
 * The run has the evaluations of ladi_sched_table_from(first_step), and everything indexed per evaluation refers to them: the guidance
 * schedule's count, the step callback's index, the trace and the step-noise steps; in->cloth_zero_from_eval too.  Its start latents are
 * k_x * resample(init) + k_n * noise_latents_dev (start_out of ladi_sched_table_from; init_noise_sigma is not applied), resampled to the run's
 * [h][w] like F.interpolate(mode="bilinear", align_corners=False) when (hs, ws) != (h, w) and copied exactly otherwise.  noisy != 0: the init is
 * taken as the loop's latents at timesteps[first_step] unchanged (k_x = 1, k_n = 0, the noise is not read) -- resuming from latents a step
 * callback exported.  The init is read once per run, on the run's stream before the loop, never by the captured graph; it must stay valid like
 * the run's other inputs.  NULL or first_step == 0 switches it off (the run is then the plain one, bit for bit).  A first_step out of range for
 * the run's scheduler and step count, or a guidance schedule / step-noise count that does not match the tail, fails the run before anything is
 * launched; hs or ws < 1 or first_step < 0 is refused here. */
int ladi_tryon_set_init(ladi_tryon* t, const float* init_latents_dev, int hs, int ws, int first_step, int noisy);
/* DDIMScheduler.step's eta, or TCDScheduler.step's eta (its gamma, [0, 1]), for the following runs (sticky per handle, default 0): > 0 adds
 * the stochastic term c_n * noise[i], which needs ladi_tryon_set_step_noise.  Only DDIM (kind 0, trailing or not) and TCD (kind 8) read it:
 * a run of any other scheduler with a non-zero eta fails, and so does a TCD run with eta > 1.  eta < 0 or non-finite: error. */
int ladi_tryon_set_eta(ladi_tryon* t, float eta);
/* per-evaluation guidance scale for the following runs (sticky per handle; copied): scales_host[i] is the scale of evaluation i and
 * in->guidance_scale is ignored while a schedule is set.  NULL or count 0 switches it off.  A run whose evaluation count is not `count`
 * fails before anything is launched (PNDM has num_inference_steps + 1 evaluations); negative or non-finite entries are an error.  The run is
 * CFG-shaped (2B samples, negative_prompt_embeds_dev required) if any entry is > 1; inside such a run an evaluation whose entry is <= 1 is
 * cond-only: the UNet runs over the B conditional samples alone and their prediction is the eps (the rule the reference applies to a whole
 * run, do_classifier_free_guidance = guidance_scale > 1).  With use_graph the loop replays two graphs, one per kind of evaluation. */
int ladi_tryon_set_guidance_schedule(ladi_tryon* t, const float* scales_host, int count);
/* guidance rescale (rescale_noise_cfg of later diffusers releases) for the following runs (sticky per handle, default 0): on every CFG
 * evaluation the guided prediction of sample b is multiplied by phi * std(cond_b) / std(guided_b) + (1 - phi), unbiased standard deviations
 * over the sample's 4 * h * w elements, no epsilon.  Cond-only evaluations and runs without CFG are not touched.  phi outside [0, 1]: error. */
int ladi_tryon_set_guidance_rescale(ladi_tryon* t, float phi);
/* how many evaluations of the last run ran cond-only, i.e. over B samples (all of them for a run without CFG) */
int ladi_tryon_cond_only_evals(ladi_tryon* t);
/* deep-feature cache (DeepCache, first level only) for the following runs (sticky per handle; copied): full_flags_host[i] != 0 runs
 * evaluation i whole (and captures the tensor ladi_unet_forward_cached describes), 0 runs it shallow at `branch` from the last capture.
 * NULL or count 0 switches it off; a plan without a 0 is the plain run bit for bit (capture stays off).  A run whose evaluation count is not
 * `count` (PNDM: num_inference_steps + 1; a strength run: the tail's), or whose flag 0 is 0, fails with -10 before anything is launched;
 * branch outside 0 .. 2 is refused here.  One promotion, decided on the host before the loop: in a CFG-shaped run a shallow evaluation over
 * all 2B samples that follows a whole evaluation which ran cond-only (so only the conditional rows were refreshed) runs whole instead; a
 * shallow cond-only evaluation is never promoted.  Nothing else is special: the cloth cut-off (cloth_zero_from_eval), a step callback's edit
 * of the latents and PNDM's double evaluation reuse the cache as it is.  Everything indexed per evaluation keeps its meaning.  With use_graph
 * the loop replays up to four graphs, {whole, shallow} x {2B samples, cond-only}.  Works with any lane count. */
int ladi_tryon_set_feature_cache(ladi_tryon* t, const unsigned char* full_flags_host, int count, int branch);
/* how many evaluations of the last run ran shallow, after promotion */
int ladi_tryon_shallow_evals(ladi_tryon* t);
/* the per-evaluation plan ladi_tryon_run makes of a run with `evals` evaluations from the scalar guidance_scale and what
 * ladi_tryon_set_guidance_schedule, _set_guidance_rescale, _set_pag and _set_feature_cache were given (a NULL table or a count of 0: not set).
 * Host arithmetic only: needs no handle and never touches the GPU.  forms_out[i] (evals bytes) is the form of evaluation i: bit 0 cond-only,
 * bit 1 shallow (after the promotion), bit 2 PAG.  Returns evals, or what the run would be refused with (-9, -10,
 * LADI_TRYON_PAG_WITH_FEATURE_CACHE) with the run's message in ladi_last_error; first_step / steps only word that message. */
int ladi_tryon_plan_forms(int evals, int first_step, int steps, float guidance_scale, const float* guidance_tab_host, int guidance_count,
                          float phi, const float* pag_tab_host, int pag_count, const unsigned char* full_flags_host, int flag_count,
                          unsigned char* forms_out);
/* keep the unmasked region for the following runs (sticky per handle; (0, 0) = off, the state of a new handle: nothing is launched for it and
 * every result stays bit for bit).  mode_bits: bit 0 latents, bit 1 pixels.
 * Latents: diffusers' 4-channel inpaint rule.  After the scheduler update of evaluation i every KEEP latent pixel is replaced by
 * k_x[i] z0 + k_n[i] noise (ladi_sched_keep_coeffs: the scheduler's add_noise at timesteps[i + 1]), after the last evaluation by z0 itself.
 * z0 = scaling_factor * mode(vae.encode(image_dev)) (one more encode per run, no RNG draw), noise = noise_latents_dev (also with an init),
 * keep = 1 - maxpool8x8(binarised mask): the pixel's whole 8x8 footprint is unmasked.  A select on the mask: generated pixels keep their bits,
 * keep pixels never see the UNet's values.  Scheduler state (PLMS cur_sample, the eps / data-prediction ring) is not blended -- what a loop
 * gets that blends scheduler.step(...).prev_sample.  The latents trace, the step callback and the next UNet input see the blended latents.
 * Pixels: the decode epilogue writes M g + (1 - M) p, g = clamp(decoded / 2 + 0.5, 0, 1), p = clamp(image / 2 + 0.5, 0, 1), M the binarised
 * mask or, with feather_sigma > 0, its separable Gaussian blur (sigma in pixels, radius ceil(3 sigma), replicate border, fp32); M == 0 / 1
 * select p / g bit for bit; fp32 and u8 output alike.  feather_sigma outside [0, 32], a feather without bit 1, or unknown bits: error. */
int ladi_tryon_set_preserve(ladi_tryon* t, int mode_bits, float feather_sigma);
/* step callback (diffusers' callback / callback_steps): after evaluation i with i % every == 0, on the run's stream, the loop's latents are
 * copied to latents_nchw_dev (caller-owned fp32 [B,4,h,w], what the modular path hands its callback), the stream is synchronised and
 * fn(user, i) runs on the calling thread.  Afterwards work queued on the run's `stream` argument is waited for, and latents_nchw_dev is copied
 * back into the loop (and into the next UNet input), so in-place edits take effect.  fn must not call back into this handle.  A non-zero
 * return aborts the run: ladi_tryon_run returns LADI_TRYON_CALLBACK_ABORTED, nothing is decoded, and the handle stays usable.  The callback
 * points sit between graph launches; with fn == NULL (off, the default) the loop runs exactly as without this call.  Sticky per handle. */
typedef int (*ladi_step_callback)(void* user, int eval_index);
#define LADI_TRYON_CALLBACK_ABORTED (-8)
int ladi_tryon_set_step_callback(ladi_tryon* t, ladi_step_callback fn, void* user, int every, float* latents_nchw_dev);
/* stage times (ms) of the last run: [0] preprocess + VAE encodes + EMASC, [1] denoising loop, [2] decode. Sync first. */
int ladi_tryon_stage_ms(ladi_tryon* t, float* out3);
/* fp16-range guard of the decode, examined WITHOUT a host round trip inside ladi_tryon_run (round 6): a run decodes once and queues the guard's flag
 * behind its last kernel.  Returns 0 if the last run's decode stayed inside the fp16 range (or nothing is pending), 1 if it did not -- that run's
 * images are invalid; with ladi_vae_set_range_shift(-1) (automatic, the default) the shift has been raised (0 -> 4 -> 8) and re-submitting the
 * batch gives the result -- and < 0 on error.  Waits for the queued flag copy (i.e. for the run to finish).  A caller that never asks is told by
 * the NEXT ladi_tryon_run, which then fails with -101 instead of running. */
int ladi_tryon_poll_overflow(ladi_tryon* t);
/* sample-group lanes of the denoising loop: the UNet forward of the 2B (CFG) or B samples runs as `lanes` independent forwards on as
 * many HIP streams inside one hipGraph (csrc/runtime.h UNetLanes).  0 = default (environment LADI_UNET_LANES, else 1); a count that
 * does not divide the sample count falls back to the default rule.  Results do not depend on it beyond fp16 rounding of other tile
 * selections.  ladi_tryon_lanes() returns the count the last run used. */
int ladi_tryon_set_lanes(ladi_tryon* t, int lanes);
int ladi_tryon_lanes(ladi_tryon* t);
/* run ONLY `iters` UNet forwards (n samples of h x w latents, context already set) bracketed by HIP events on `stream`
 * and return the average milliseconds per forward (synchronises). Used by bench.py for the roofline figure. */
int ladi_unet_time_forward(ladi_unet* u, int n, int h, int w, int iters, float* avg_ms, void* stream);
/* Supported ABI (what tools/bench_feature_cache.py times the shallow forward with): the same measurement of a forward in feature-cache
 * mode `mode` (ladi_unet_forward_cached: 1 whole + capture, 2 shallow at `branch`; 0 is ladi_unet_time_forward) against a scratch cache of
 * zeros: the launch sequence and shapes are those of the real thing */
int ladi_unet_time_forward_cached(ladi_unet* u, int n, int h, int w, int iters, int mode, int branch, float* avg_ms, void* stream);
/* the same measurement of the forward as the denoising loop runs it: `lanes` independent sample groups on as many HIP streams (0 =
 * the loop's own choice, LADI_UNET_LANES or 1; must divide n), replayed from one hipGraph with `lanes` parallel branches when
 * use_graph != 0.  Runs on an internal stream fenced against `stream`; synchronises. */
int ladi_unet_time_forward_lanes(ladi_unet* u, int n, int h, int w, int iters, int lanes, int use_graph, float* avg_ms, void* stream);
/* FreeU (diffusers UNet2DConditionModel.enable_freeu, same argument order; sticky, off at creation).  on != 0: before every concatenation
 * cat([hidden, skip]) of up_blocks.0 (s1, b1) and up_blocks.1 (s2, b2) the first half of the hidden state's channels is multiplied by b
 * and the skip goes through diffusers' fourier_filter(threshold = 1, scale = s) -- one extra launch per site, 2 * (layers_per_block + 1)
 * per whole forward; a shallow forward of the feature cache has no such site.  Every entry that runs this UNet honours it (forward,
 * forward_cached, time_forward*, ladi_tryon_run, whose captured graphs are keyed on it).  on == 0 ignores the values and launches
 * exactly the plain forward.  A null handle or a non-finite value returns -1 with a message. */
int ladi_unet_set_freeu(ladi_unet* u, int on, float s1, float s2, float b1, float b2);
/* Perturbed-attention guidance (diffusers PAGMixin: pag_scale, pag_adaptive_scale, pag_applied_layers).  A PAG evaluation has one more
 * sample group behind the conditional one, with the conditional group's inputs and context; in the SELECTED transformer blocks the
 * self-attention (attn1) of those perturbed samples has the identity as its attention map, i.e. its output is to_out(to_v(norm1(x))):
 * no attention is launched for them, one 16-byte copy kernel moves V into the attention output.  attn2, the feed-forward, every other block
 * and every other sample are untouched.
 * The transformer blocks are numbered in execution order: bits 0 .. 3L-1 down_blocks.{0,1,2}.attentions.{0..L-1}, bit 3L mid_block, bits
 * 3L+1 .. 6L+3 up_blocks.{1,2,3}.attentions.{0..L} (L = layers_per_block; 16 blocks for L = 2, the mid block is bit 6).
 * ladi_unet_pag_layer_count: the number of blocks.  ladi_unet_set_pag_layers: sticky; the state of a new handle is the mid block alone
 * (diffusers' default); a mask of 0 or with bits beyond the count returns -1 with a message and changes nothing.  The mask has no effect on
 * a forward without perturbed samples.  ladi_unet_pag_layers: the current mask (0 for a null handle).
 * ladi_unet_forward_pag: ladi_unet_forward over the samples [sample0, sample0 + n) of the context batch (ladi_unet_set_context); samples
 * whose index in that batch is >= pag_first are perturbed (pag_first >= sample0 + n: none, the plain forward bit for bit; <= sample0:
 * all, and the selected blocks launch no self-attention).  The unperturbed samples' results do not depend on the others. */
int ladi_unet_pag_layer_count(const ladi_unet* u);
int ladi_unet_set_pag_layers(ladi_unet* u, unsigned layer_mask);
unsigned ladi_unet_pag_layers(const ladi_unet* u);
int ladi_unet_forward_pag(ladi_unet* u, const void* sample_dev, int dtype, int n, int h, int w, float timestep, void* out_dev, int out_dtype,
                          int sample0, int pag_first, void* stream);
/* ---- LoRA adapters (DESIGN.md "LoRA").  The weights of a UNet stay where they are; an adapter is merged onto them on the device:
 *   W = fp16(base + sum_a weight_a * alpha_a / rank_a * up_a down_a)    (fp32 arithmetic, one rounding, always from the pristine copy)
 * so captured graphs, tile selections and arenas stay valid and the forward launches exactly what it launched before.
 * Targets are the diffusers module names of every conv and linear of the UNet (conv_in, conv_out, time_embedding.linear_1 / 2, every
 * resnet's conv1, conv2, conv_shortcut and time_emb_proj, the down- and upsampler convs, and per transformer proj_in, attn1.to_q / to_k /
 * to_v / to_out.0, attn2.to_q / to_k / to_v / to_out.0, ff.net.0.proj, ff.net.2, proj_out); norms and biases are not targets.
 *
 * ladi_unet_lora_load: `ws` holds <module>.lora_down.weight ([r, in] or [r, in, k, k]), <module>.lora_up.weight ([out, r] or [out, r, 1, 1])
 * and optionally <module>.alpha (one number; default r).  Everything is checked first -- unknown module, shapes against the target, r in
 * [1, 256], a name already loaded, more than 8 loaded adapters, any other key -- and on an error nothing has changed.  The factors go to the
 * device in fp32; the first time a packed weight is touched a pristine fp16 copy of it is kept (at most one extra copy of the touched
 * weights, for the life of the UNet).  Loading does not activate.
 * ladi_unet_set_adapters: the active set, in this order (count = 0: none, every weight is restored bit for bit).  The live weights are
 * rewritten in place, so the call first waits for the whole device (work on any stream may be reading them).  Every block touched by
 * the new or the previous set is merged again from its pristine copy on `stream`; the cross-attention K/V cache is dropped (a forward
 * needs a new ladi_unet_set_context and says so), the stand-alone feature cache is dropped and the re-packed operands of the fused
 * sub-blocks are packed again.  The call then reads a device counter of merged values outside the fp16 range (one synchronisation of
 * `stream`): if there is one, the previous set is merged back and the error names the first such module.
 * ladi_unet_lora_delete: refused while the adapter is active.  ladi_unet_lora_count / ladi_unet_lora_name: the loaded adapters, in load
 * order (-1 / NULL for a null handle or a bad index).  ladi_unet_lora_active: the active set's size; the first min(size, cap) names
 * (valid until the next change) and weights are written.
 * ladi_unet_export_weight: the LIVE value of a diffusers .weight key of a target, in diffusers layout ([out][in][kh][kw], fp32 holding
 * fp16 values), into host_out[cap]; returns the element count (host_out == NULL: the count alone), -1 on an error.  Synchronises. */
int ladi_unet_lora_load(ladi_unet* u, const char* name, const ladi_weights* ws);
int ladi_unet_set_adapters(ladi_unet* u, const char* const* names, const float* weights, int count, void* stream);
int ladi_unet_lora_delete(ladi_unet* u, const char* name);
int ladi_unet_lora_count(const ladi_unet* u);
const char* ladi_unet_lora_name(const ladi_unet* u, int i);
int ladi_unet_lora_active(const ladi_unet* u, const char** names_out, float* weights_out, int cap);
long long ladi_unet_export_weight(ladi_unet* u, const char* key, float* host_out, long long cap);
/* ---- IP-Adapter image prompt (DESIGN.md "IP-Adapter"; diffusers load_ip_adapter / set_ip_adapter_scale / ip_adapter_image_embeds).  With an
 * image context set, attn2 of every transformer block computes
 *   to_out(softmax(q k_text^T / 8) v_text + s_block * softmax(q k_ip^T / 8) v_ip),  k_ip | v_ip = (to_k_ip | to_v_ip)(tokens)
 * with tokens = LayerNorm(Linear(image_embeds)).reshape(n, N, cross_dim).  The image K/V are hoisted out of the denoising loop like the
 * text K/V; the per-evaluation work is one launch per block (csrc/ip_adapter.hip) between the attention and to_out.
 * ladi_unet_ip_adapter_load: `ws` holds image_proj.proj.weight [N * cross_dim, E], image_proj.proj.bias, image_proj.norm.weight / .bias and,
 * for every transformer block, <block>.transformer_blocks.0.attn2.processor.to_k_ip.weight and ...to_v_ip.weight ([C, cross_dim], no bias),
 * <block> = down_blocks.i.attentions.j, mid_block.attentions.0, up_blocks.i.attentions.j.  N comes from the projection's rows, E from its
 * columns.  Everything is checked first -- every block present, the shapes, N in [1, 64], E % 8, no other key -- and on an error nothing has
 * changed.  One adapter per UNet: a second load is refused until ladi_unet_ip_adapter_unload (which waits for the device and drops the
 * weights, the scales and the image context).  Loading activates nothing.  The weights are fp16 on the device: about 51 MB of to_k_ip /
 * to_v_ip at the released architecture, 8 MB of projection at N = 4; the image K/V are n * N rows of 2C halves per block, 3.2 MB for n = 16, N = 4.
 * ladi_unet_ip_adapter_info: 1 with a loaded adapter (its N and E written), 0 without.
 * ladi_unet_set_ip_scale: `count` == ladi_unet_pag_layer_count(u) floats, one per block in the execution order PAG's mask uses.  Sticky; a
 * new adapter starts with every scale 1.0.  A block with scale 0 launches nothing for the image term.  A wrong count, a non-finite value or
 * no loaded adapter returns -1 and changes nothing.  ladi_unet_ip_scale: the current scales (returns the block count).
 * ladi_unet_set_ip_context: embeds_dev fp16 [n][E] -> the projection, the per-token LayerNorm (eps 1e-5) and one GEMM per block into that
 * block's image K/V [n][N][2C], asynchronous on `stream`.  ladi_unet_set_ip_tokens: finished tokens fp16 [n][N][cross_dim] instead (adapter
 * variants with another projection network); its N, 1 .. 64, may differ from the loaded projection's.  ladi_unet_clear_ip_context: no image
 * context; the forward is then the plain one, launch for launch.
 * A forward reads the image K/V rows of its own samples (sample0), as it reads the text K/V; an image context whose n is not the text
 * context's fails with a "batch mismatch" error.  Under LADI_XF_FUSE a block with an image term takes the un-fused chain.  Shallow forwards
 * of the feature cache skip the blocks they skip; PAG perturbs attn1 only.  ladi_unet_set_adapters (LoRA) leaves the image K/V alone: LoRA
 * has no to_k_ip / to_v_ip target.
 * Plus adapters: when `ws` holds image_proj.latents, image_proj.* is a Resampler in its original key layout (ladi_resampler_create above,
 * every key prefixed with image_proj.) instead of the Linear + LayerNorm; its out_dim has to be cross_dim, and its limits are checked like
 * everything else, before anything changes.  ladi_unet_ip_adapter_load builds it with dim_head 64, ladi_unet_ip_adapter_load_ex with the
 * given one (ignored for a plain adapter).  ladi_unet_ip_adapter_info then reports the Resampler's N and E, ladi_unet_ip_adapter_is_plus
 * returns 1 (0: plain or none).  ladi_unet_set_ip_context_seq: hidden_dev fp16 [n][T][E] (the encoder's penultimate hidden states)
 * -> the Resampler -> the per-block K/V GEMMs, asynchronous on `stream`; on a plain adapter it is refused with a message, as
 * ladi_unet_set_ip_context is on a Plus adapter.  ladi_unet_set_ip_tokens works with both. */
int ladi_unet_ip_adapter_load(ladi_unet* u, const ladi_weights* ws);
int ladi_unet_ip_adapter_load_ex(ladi_unet* u, const ladi_weights* ws, int image_proj_dim_head);
int ladi_unet_ip_adapter_is_plus(const ladi_unet* u);
int ladi_unet_set_ip_context_seq(ladi_unet* u, const void* hidden_dev, int n, int T, void* stream);
int ladi_unet_ip_adapter_unload(ladi_unet* u);
int ladi_unet_ip_adapter_info(const ladi_unet* u, int* tokens, int* embed_dim);
int ladi_unet_set_ip_scale(ladi_unet* u, const float* scales, int count);
int ladi_unet_ip_scale(ladi_unet* u, float* scales_out, int cap);
int ladi_unet_set_ip_context(ladi_unet* u, const void* embeds_dev, int n, void* stream);
int ladi_unet_set_ip_tokens(ladi_unet* u, const void* tokens_dev, int n, int N, void* stream);
int ladi_unet_clear_ip_context(ladi_unet* u);
/* measurement switch (tools/bench_ip_adapter.py): route 0 (default, shipped) computes the image term with csrc/ip_adapter.hip, route 1 with
 * the kernels that existed before it -- the flash attention over the N image keys into a scratch tensor, then a scaled add (two roundings
 * instead of one).  Sticky; -1 for another value. */
int ladi_unet_set_ip_route(ladi_unet* u, int route);
/* Image embeddings of the following runs (sticky per handle; the pointers are read by every run, on its stream): fp16 [B][E] each, E the
 * loaded adapter's.  negative_embeds_dev NULL means zeros (diffusers' zeros_like; the projection still runs on them, so the unconditional
 * tokens are LayerNorm(bias)).  embeds_dev NULL switches the image prompt off: the run clears the UNet's image context.  A run assembles
 * [neg ; pos] (CFG-shaped), [neg ; pos ; pos] (with PAG) or [pos] into a buffer of its own and sets the UNet's image context right after the
 * text context.  A run on a UNet without a loaded adapter fails with LADI_TRYON_IP_NO_ADAPTER before anything is launched; a run with every
 * scale 0 is the plain run bit for bit.  The captured graphs are keyed on the image term: on / off, N, the image K/V and every scale. */
#define LADI_TRYON_IP_NO_ADAPTER (-13)
int ladi_tryon_set_ip_adapter(ladi_tryon* t, const void* embeds_dev, const void* negative_embeds_dev);
/* The same for a Plus adapter: hidden states of the image encoder, fp16 [B][T][E] each (hidden_states[-2]; negative_hidden_dev NULL means
 * zeros).  Sticky; this setter and ladi_tryon_set_ip_adapter replace each other, and hidden_dev NULL switches the image prompt off.  A run
 * assembles the same groups with rows of T * E halves and hands them to ladi_unet_set_ip_context_seq, i.e. the Resampler runs once per
 * run, outside the captured graphs; graph key, lanes, feature cache, PAG and SAG behave as with the plain adapter.  A run whose kind of
 * input does not fit the loaded adapter -- hidden states with a plain adapter, embeddings with a Plus adapter -- fails with
 * LADI_TRYON_IP_ADAPTER_KIND before anything is launched. */
#define LADI_TRYON_IP_ADAPTER_KIND (-19)
int ladi_tryon_set_ip_adapter_seq(ladi_tryon* t, const void* hidden_dev, const void* negative_hidden_dev, int T);
/* PAG scales of the following runs (sticky per handle; copied): scales_host[i] = s_i of evaluation i.  NULL or count 0 switches it off; a
 * table of zeros is the plain run bit for bit (nothing is allocated or launched for it).  With any s_i > 0 the run has the third sample group
 * ([uncond ; cond ; perturbed], or [cond ; perturbed] without CFG; context [neg ; pe ; pe]) and the guided prediction of an evaluation with
 * s_i > 0 is u + g_i (c - u) + s_i (c - p), or c + s_i (c - p) without CFG and in a cond-only evaluation; guidance rescale acts on the
 * three-term sum of CFG evaluations.  An evaluation with s_i == 0 runs without the perturbed group.  The blocks are the UNet's
 * (ladi_unet_set_pag_layers).  A run whose evaluation count is not `count` fails with -9 before anything is launched, like a guidance
 * schedule of the wrong length; a negative or non-finite entry returns -1 here.  NOT supported together with the feature cache: a run with
 * a positive entry and a feature-cache plan fails with LADI_TRYON_PAG_WITH_FEATURE_CACHE before anything is launched.  With use_graph the
 * loop replays up to two more graphs (PAG evaluation over all groups, and over cond + perturbed); works with any lane count. */
#define LADI_TRYON_PAG_WITH_FEATURE_CACHE (-12)
int ladi_tryon_set_pag(ladi_tryon* t, const float* scales_host, int count);
/* ---- Self-attention guidance (diffusers StableDiffusionSAGPipeline, sag_scale; DESIGN.md "Self-attention guidance").
 * The SAG map: for the self-attention (attn1) of mid_block.attentions.0's transformer block, per sample,
 *   s[j] = sum_i mean_h softmax_j(q_i k_j / 8)     (fp32, the column sums of the attention map)     m[j] = s[j] > 1
 * over the T = hm * wm tokens of the mid block (ladi_unet_sag_tokens: three times ceil(x / 2) of the latent sides).
 * ladi_unet_set_sag_capture: sticky, off at creation.  On: every forward of this UNet (forward, forward_pag, forward_cached whole, the fused
 * loop) runs csrc/sag.hip's sag_map right after that block's Q / K projection, for all its samples, into buffers of the UNet's at the rows
 * of the samples' indices in the context batch.  Two small launches; the forward's output does not change by a bit.  Off: nothing is
 * allocated or launched.  Captured graphs are keyed on it.
 * ladi_unet_sag_map: what the last capturing forward left, rows [0, n) of the context batch: s_out_dev fp32 [n][T], m_out_dev bytes [n][T]
 * (either may be NULL).  T has to be the last capture's.  Waits for the device.
 * ladi_tryon_set_sag: the scale of the following runs (sticky per handle; 0 = off, the state of a new handle: the run is the plain run bit
 * for bit).  With a scale > 0 EVERY evaluation is
 *   first forward (as today, capturing the map) -> sag_degrade -> second forward over B samples -> combine + scheduler step
 * where, with a = alphas_cumprod[t], b the base prediction (the unconditional one in a CFG evaluation, else the conditional one) and m the
 * base group's mask,   x0 = (x - sqrt(1 - a) b) / sqrt(a),  x0d = blur9(x0) where nearest-upsample(m) is 1 else x0,
 * xd = sqrt(a) x0d + sqrt(1 - a) b;  the second forward sees xd in channels 0..3 and the base group's other channels, context rows and image
 * tokens, and gives d;  e = [u + g (c - u) | c] + sag_scale (b - d), guidance rescale acting on the whole sum.  blur9: depthwise 9 x 9
 * Gaussian, sigma 1, reflect padding 4.  All of it inside the same captured graph; the scale is read from device memory, so another value
 * replays the same graphs, while switching between 0 and > 0 drops them.  Works at any lane count (the second forward runs on the lanes
 * that divide B).  Composes with guidance schedules, rescale, strength, preserve-unmasked, callbacks, FreeU, LoRA, IP-Adapter and token merging
 * on the outer levels.  Refused before anything is launched, with a message:
 *   LADI_TRYON_SAG_WITH_FEATURE_CACHE  a feature-cache plan is set (shallow evaluations do not run the mid block)
 *   LADI_TRYON_SAG_WITH_PAG            a positive PAG scale is set
 *   LADI_TRYON_SAG_TOME_MID            token merging is configured so that the mid block merges
 *   LADI_TRYON_SAG_SCHEDULER           Euler, Euler-ancestral or LMS (sigma space: pred_x0 / add_noise do not describe them)
 *   LADI_TRYON_SAG_SMALL_LATENTS       latents under 5 x 5
 * ladi_tryon_plan_forms_sag: ladi_tryon_plan_forms with the SAG state -- the scale, the scheduler code, the latent size and whether token
 * merging merges in the mid block -- so the refusals above are reported without a GPU.  A SAG run's evaluation count and forms are the
 * plain run's. */
#define LADI_TRYON_SAG_WITH_FEATURE_CACHE (-14)
#define LADI_TRYON_SAG_WITH_PAG (-15)
#define LADI_TRYON_SAG_TOME_MID (-16)
#define LADI_TRYON_SAG_SCHEDULER (-17)
#define LADI_TRYON_SAG_SMALL_LATENTS (-18)
int ladi_unet_set_sag_capture(ladi_unet* u, int on);
int ladi_unet_sag_tokens(const ladi_unet* u, int h, int w, int* hm, int* wm);
int ladi_unet_sag_map(ladi_unet* u, float* s_out_dev, unsigned char* m_out_dev, int n, int T);
int ladi_tryon_set_sag(ladi_tryon* t, float sag_scale);
/* how many hipGraph captures this handle has made over its life (-1 for a null handle): a run that replays the graphs it has adds none */
long long ladi_tryon_graph_captures(ladi_tryon* t);
int ladi_tryon_plan_forms_sag(int evals, int first_step, int steps, float guidance_scale, const float* guidance_tab_host, int guidance_count,
                              float phi, const float* pag_tab_host, int pag_count, const unsigned char* full_flags_host, int flag_count,
                              float sag_scale, int scheduler, int lat_h, int lat_w, int tome_mid_merges, unsigned char* forms_out);

/* per-launch HIP-event timing of the implicit-GEMM kernel family (the dominant kernel): enable, run any entry point,
 * then collect: out[cfg*3 + {0,1,2}] = {total ms, algorithmic FLOP = 2*P*Q*K, launches} for tile configuration cfg = 1..ladi_igemm_cfg_count()
 * (igemm tile shapes, split-K variants, the X-stationary linear kernel; table in csrc/igemm.hip), index 0 = all; entries beyond
 * n_out are dropped. collect() synchronises and clears the records. */
/* measured tile-shape selection (default on): the first launch of a new problem shape outside a stream capture times the
 * admissible tile configurations and caches the fastest; off = static cost model */
void ladi_igemm_set_autotune(int on);
/* split-K launches combine their K slices inside the launch (last-arriving slice of a tile runs the fused epilogue; csrc/igemm_common.h);
 * on = 1 switches to the separate reduce pass of rounds 1-3 (A/B measurements, parity tests of one form against the other) */
void ladi_igemm_set_splitk_two_pass(int on);
void ladi_profile_igemm_enable(int on);
int ladi_profile_igemm_collect(double* out, int n_out);
/* the same records grouped by the exact kernel symbol rocprofv3 reports (the X-stationary kernel has several): text lines
 * "symbol\tms\tflop\tlaunches\n" into buf (at most n bytes, NUL-terminated); returns the untruncated length.  Call BEFORE collect(). */
int ladi_profile_igemm_symbols(char* buf, int n);
/* number of tile configurations (valid ids 1..count) and the kernel symbol configuration `cfg` launches, as rocprofv3 names it
 * (split-K variants share the symbol of their base tile); "" for an unknown id.  The string is owned by the library. */
int ladi_igemm_cfg_count(void);
/* what the LAST implicit-GEMM launch of this process did, as recorded by the launcher that computed its grid (not a restatement of the rule):
 * out[0] kernel family (1 ring, 2 igemm8, 3 loader / consumer, 4 halo, 5 X-stationary linear), out[1] tile_map as the kernel received it
 * (0 plain, 1 pixel tiles over the XCDs, 2 channel tiles over the XCDs, 3 | G << 4 weight-slice-major with groups of G pixel tiles),
 * out[2] split-K factor (1 = none), out[3] workgroups per grid plane (0 for family 5).  A launch with tile_cfg = 0 that tunes first reports
 * the launch that produced the output (the last one).  Not thread-safe, like the handles. */
int ladi_igemm_last_launch(int out[4]);
const char* ladi_igemm_cfg_symbol_name(int cfg);
/* Host-only introspection of the tile selection a launch with tile_cfg = 0 makes (ladi_igemm_desc is declared below).  None of these launches
 * anything or dereferences an operand pointer; only null / non-null is looked at.
 *   tune_key:       the key the launch would look up, key = {P, Q, K, C0, C1, Wo, flags, batch}; returns 0, or the launch's own argument refusal
 *                   (-1 .. -6, -18, -19, -20) and leaves key alone.  The launch computes its key with the same function.
 *   tune_lookup:    the configuration the selection table holds for key (the shipped tune_gfx950.txt, LADI_TUNE_CACHE and this process's
 *                   measurements, loaded exactly as a launch loads them), 0 = none
 *   tune_put:       process-local: set the table's entry for key (cfg = 0 erases it); returns the previous value (0 = none), -1 for a bad cfg
 *   cfg_admissible: 1 if the launcher's admission rule accepts configuration cfg for this launch (strict = 1: as the tuner and a table hit
 *                   are judged; strict = 0: as the cost model's candidates are), else 0
 *   last_selection: out = {configuration launched, source} of the last launch made from outside the library: source 0 = tile_cfg given,
 *                   1 = table, 2 = measured by this launch, 3 = cost model (also after an inadmissible table hit), 4 = the fixed list of
 *                   X-stationary forms a gn_ss launch (or one whose pixel operand is beyond every tile's reach, rc -20) falls back to.  The tuner's own timing launches do not overwrite it.
 *   launch_log:     on = 1 clears the log and starts recording, on = 0 stops (the log stays readable).  While on, every launch made from
 *                   outside the library (product call sites and ladi_op_igemm alike; not the tuner's timing launches) adds one text line per
 *                   DISTINCT launch: "name=value" pairs for every integer field of the descriptor, the four batch strides, batch,
 *                   ops = bit mask of the operands present (1 src1, 2 bias, 4 rowadd, 8 rowadd_idx, 16 res0, 32 res1, 64 mask, 128 stats,
 *                   256 ln_gamma, 512 ln_scratch, 1024 gn_ss, 2048 bias_mul not in {0, 1}, 4096 out_scale != 1), key = the eight key integers,
 *                   cfg, src (as last_selection), rc, last = the four ladi_igemm_last_launch values, px = stats_row_px, n = repeat count.
 *                   No pointer and no value is recorded.  launch_log_read has the calling convention of ladi_profile_igemm_symbols.
 *   A launch that is refused AFTER its configuration was chosen (rc -2, -7 .. -9, -12 .. -17, -20 for its configuration) counts: last_selection reports its choice,
 *   the log holds its line with that rc, and ladi_igemm_last_launch reports family 0.  A launch refused for its arguments (the codes tune_key
 *   returns) has no key and no selection: it is not logged and leaves last_selection alone. */
int ladi_igemm_tune_lookup(const int key[8]);
int ladi_igemm_tune_put(const int key[8], int cfg);
int ladi_igemm_last_selection(int out[2]);
void ladi_igemm_launch_log(int on);
int ladi_igemm_launch_log_read(char* buf, int n);

/* ---------------------------------------------------------------------------------------------------------------
 * Op-level entry points (kernel parity tests; NHWC fp16 device tensors)
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    /* ups = 1: nearest upsample folded into the gather, stride 1 only.  The Hs x Ws source is stretched to the logical
     * (Ho + ksize - 1 - 2 pad) x (Wo + ksize - 1 - 2 pad) image -- Ho x Wo for a 3x3 pad-1 conv.  Twice the source is nearest-2x (the
     * meaning of every descriptor with Ho == 2 Hs); any other size maps output index d to min(floor(d * (in / out)), in - 1) in fp32, as
     * F.interpolate(size=..., mode="nearest").  Only the generic tile forms take non-2x sizes; the halo forms refuse them. */
    const void* src0; const void* src1; int C0, C1, ld0, ld1, Hs, Ws, Ho, Wo, P, ksize, stride, pad, ups;
    const void* W; int Q, K, ldw; long long bs_src0, bs_w, bs_out, bs_res;
    const void* bias; int bias_per_pixel; const float* rowadd; const int* rowadd_idx; int rowadd_stride; int act; float out_scale;
    const void* res0; const void* res1; int ldr0, ldr1; const void* mask; void* out; int ldo; int out_f32;
    float* stats; int stats_groups; int splitk, tile_map /* both ignored: set by the launcher */;
    const void* ln_gamma; const void* ln_beta; float ln_eps; float bias_mul /* multiplier of bias, 0 = 1 */; void* ln_scratch;
    float* sk_ws; int* sk_cnt;   /* both ignored: set by the launcher (in-launch split-K combine) */
    const float* gn_ss; int gn_hw; /* optional GroupNorm affine of the pixel operand: [n][C0][2] floats (scale, shift), pixels per sample
                                      (multiple of 32); K = 320 / 640 projections without residual / GEGLU only */
    /* optional LayerNorm of the pixel operand (single source, 1x1): fused into the X-stationary linear kernel where the tuner finds that
       faster, else run as its own kernel into ln_scratch ([P][C0] fp16, caller-provided; null = only the fused form is admissible) */
    /* The epilogue: t = act(acc + bias * bias_mul + rowadd), out = fp16(fp16(t * out_scale) + res0 + res1) * (1 - mask); bias is indexed by
       output channel, or by pixel when bias_per_pixel.  batch > 1 runs `batch` problems whose src0 / W / out / res0 and res1 lie bs_src0 / bs_w /
       bs_out / bs_res elements apart (0 = shared).  Two combinations are refused, for every tile_cfg (0 included):
         rc -18: batch > 1 with a second source (src1 / C1): there is no batch stride for it;
         rc -19: out_f32 with an activation, rowadd, res0, res1 or mask: the fp32 store is (acc + bias * bias_mul) * out_scale only.
       The size limit of the pixel operands and the weight (rc -20).  The tiled kernels (ring, igemm8, loader / consumer) gather src0 / src1
       through 32-bit byte offsets from the first sample a workgroup's pixel tile touches, so what a tile of bp pixels can reach,
           span = 2 ((ns Hs Ws + Hs Ws - 1 + back_px) ld + C) bytes,   back_px = ups ? 0 : pad Ws + pad,
           ns = min((Ho Wo - gcd(bp, Ho Wo) + bp - 1) / (Ho Wo), samples - 1)   (0 when bp divides Ho Wo),
       has to stay below 0x7FFFFFFF for each source (ld = ld0 / ld1, C = C0 / C1), and so has the weight's 2 ((Q - 1) ldw + K).  The tensor as
       a whole may be of any size: only a sample (Hs Ws ld) counts, twice that where a tile straddles two samples.  A configuration whose span
       reaches the limit is not admissible (ladi_igemm_cfg_admissible returns 0, tile_cfg = 0 never selects it and prefers one whose tiles lie
       inside single samples); an explicit tile_cfg of that kind, and tile_cfg = 0 when no configuration is left, return rc -20 and launch
       nothing; ladi_last_error then names P, Hs Ws, ld and the span.  When already a single sample (or the weight) is out of reach and the
       launch is not one the X-stationary kernel takes (which addresses its pixel operand with 64 bits), -20 is an argument refusal like -18
       and -19: ladi_igemm_tune_key returns it too.  The halo forms keep their stricter rule (the whole tensor below 0x7FFFFFFF bytes, rc -16
       for an explicit tile_cfg).  out, res0, res1, mask, the statistics rows and every batch stride are addressed with 64 bits: no limit. */
} ladi_igemm_desc;
int ladi_op_igemm(const ladi_igemm_desc* d, int batch, int tile_cfg, void* stream);
int ladi_igemm_tune_key(const ladi_igemm_desc* d, int batch, int key[8]);
int ladi_igemm_cfg_admissible(const ladi_igemm_desc* d, int batch, int cfg, int strict);
int ladi_op_group_norm(const void* src0, int C0, const void* src1, int C1, int n, int HW, int groups, const void* gamma,
                       const void* beta, float eps, int silu, const void* add, void* out, float* stats_scratch, void* stream);
/* ladi_op_igemm, and *stats_row_px = pixels per row of the partial statistics the launch wrote into d->stats: [n HW / px][Q][2] floats (sum, sum
 * of squares of the values as stored), rows [s HW / px, (s + 1) HW / px) belonging to sample s; 0 = none were written and d->stats is untouched
 * (no d->stats, the X-stationary kernel, HW % px != 0, GEGLU, batch > 1, fp32 output) */
int ladi_op_igemm_stats(const ladi_igemm_desc* d, int batch, int tile_cfg, int* stats_row_px, void* stream);
/* ladi_op_group_norm whose sources bring such rows: partK = source K's rows of pxK pixels each; pxK = 0: the source has none (its statistics
 * are taken from the data).  Runs the dispatch every model runs for the same rows.  pxK > 0 with HW % pxK != 0 or a null partK is refused
 * before anything is launched. */
int ladi_op_group_norm_rows(const void* src0, int C0, const float* part0, int px0, const void* src1, int C1, const float* part1, int px1, int n,
                            int HW, int groups, const void* gamma, const void* beta, float eps, int silu, const void* add, void* out,
                            void* stream);
int ladi_op_layer_norm(const void* x, const void* gamma, const void* beta, float eps, int rows, int C, void* out, void* stream);
/* the same on strided rows: x [rows][ldx], out [rows][ldo] (ldx, ldo >= C, multiples of 8; columns [C, ld) are neither read nor written) */
int ladi_op_layer_norm_ld(const void* x, int ldx, const void* gamma, const void* beta, float eps, int rows, int C, void* out, int ldo,
                          void* stream);
/* Fused sub-blocks of diffusers' BasicTransformerBlock on the 320-channel level (5 heads of 64), fp16 operands in torch layout:
 *   xattn: out = x + to_out(softmax(to_q(LayerNorm(x)) K^T / 8) V) with kv = [n][L][640] rows (K | V of the context, L <= 96), x / out [n*T][320],
 *          T % 128 == 0 (norm2 / attn2 of the block: tryon_pipe.py:732 -> UNet2DConditionModel -> Transformer2DModel);
 *   ff:    out = x + W2 ((u + bu) * gelu(g + bg)) + bo with (u | g) = W1 LayerNorm(x), W1 / b1 in the GEGLU packing of ladi_op_igemm (32-row blocks
 *          alternate value | gate rows), w2 = [320][1280], P % 128 == 0 (norm3 / ff).  One launch each (ladi_vton_amd/csrc/xf_fused.hip). */
int ladi_op_xattn_block(const void* x, const void* ln_gamma, const void* ln_beta, float eps, const void* wq, const void* kv, int L, const void* wo,
                        const void* bo, int n, int T, void* out, void* stream);
int ladi_op_ff_block(const void* x, const void* ln_gamma, const void* ln_beta, float eps, const void* w1_geglu, const void* b1_geglu, const void* w2,
                     const void* bo, int P, void* out, void* stream);
/* flash attention on heads of 64 (ladi_op_attention, ladi_op_attention_causal).  Size limit: the keys of ONE sample are streamed through 32-bit
 * byte offsets from that sample's base, so 2 ((Nk - 1) max(ldk, ldv) + 64) has to stay below 0x7FFFFFFF; a launch beyond that returns -3 with a
 * ladi_last_error text and launches nothing.  q / o rows and the four sample strides are addressed with 64 bits: any size.  The generic and the
 * wide kernel address everything with 64 bits. */
int ladi_op_attention(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq,
                      long long sk, long long sv, long long so, int n, int heads, int Nq, int Nk, float scale, void* stream);
/* same with causal = 1: query i attends to keys <= i (the CLIP text encoder's mask; Nq == Nk) */
int ladi_op_attention_causal(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq,
                             long long sk, long long sv, long long so, int n, int heads, int Nq, int Nk, float scale, int causal,
                             void* stream);
/* heads of dimension head_dim in {64, 80, 96, 128} at column offset h*head_dim (ViT-H: 80) */
int ladi_op_attention_generic(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq,
                              long long sk, long long sv, long long so, int n, int heads, int head_dim, int Nq, int Nk, float scale,
                              void* stream);
/* ONE wide head (head_dim 128 / 256 / 512) — the VAE mid-block AttentionBlock (diffusers 0.14; src/models/vae.py:66-75 builds it through
 * UNetMidBlock2D): flash-style, scores never materialised.  q, k: [n][N][ld]; vt = V TRANSPOSED [n][head_dim][ldvt >= Nk]; ldvt % 4 == 0, any Nk */
int ladi_op_attention_wide(const void* q, const void* k, const void* vt, void* o, int ldq, int ldk, int ldvt, int ldo, long long sq,
                           long long sk, long long svt, long long so, int n, int head_dim, int Nq, int Nk, float scale, void* stream);
/* glue between the TPS network and the refinement UNet (src/inference.py:242-260), NCHW planes, dtype 0 fp32 / 1 fp16 in and out:
 * torchvision.transforms.functional.resize(x, size, BILINEAR, antialias=True) over `planes` = B*C images of H x W */
int ladi_op_resize_bilinear_aa(const void* src, int dtype, int planes, int H, int W, void* dst, int out_dtype, int Ho, int Wo, void* stream);
/* F.grid_sample(x [B,C,H,W], grid fp32 [B,Ho,Wo,2], mode bilinear, padding_mode "border", align_corners False) -> [B,C,Ho,Wo] */
int ladi_op_grid_sample_border(const void* src, int dtype, int B, int C, int H, int W, const float* grid, int Ho, int Wo, void* dst,
                               int out_dtype, void* stream);
/* shader-clock probe for the bench's roofline bookkeeping: one wave spins for `wall_ticks_100mhz` ticks of the constant 100 MHz counter
 * (at most 10^8 = 1 s) on `stream` -- a side stream, next to the work being measured -- and writes {shader cycles, wall ticks} to
 * out2_dev (2 x uint64, device): cycles / ticks * 100 = the MHz the chip sustained under that load */
int ladi_clock_probe(unsigned long long wall_ticks_100mhz, unsigned long long* out2_dev, void* stream);
/* CLIP image pre-processing of the in-shop cloth in one pass (src/inference.py:268-272): v = resize((x + 1) / 2, (size, size), antialias)
 * .clamp(0, 1), then the processor's 8-bit round trip v = floor(v * 255) / 255, then (v - mean[c]) / std[c]; src [B,3,H,W] in [-1,1]
 * (dtype 0 fp32 / 1 fp16), dst fp16 [B,3,size,size]; mean3 / std3 host.
 * The round trip is what CLIPImageProcessor of the pinned transformers 4.27.3 (environment.yml:92) does to a FLOAT32 image on its way
 * through to_pil_image -- i.e. the reference's default run (inference.py:186: weight_dtype = float32 unless --mixed_precision is given).
 * It is applied for either input dtype: with --mixed_precision fp16 the reference hands the processor a float16 array, which 4.27.3's
 * to_pil_image does not recognise as floating point (its isinstance test lists float / np.float32 / np.float64 only) and truncates
 * without the x255 rescale -- a reference-side accident this library does not reproduce; 4.27.3 is not installable in the build image
 * (5.x is), so neither branch could be run against the real processor here. */
int ladi_op_clip_preprocess(const void* src, int dtype, int B, int H, int W, int size, const float* mean3, const float* std3, void* dst_f16,
                            void* stream);
/* NHWC fp16 helpers of the refinement UNet: 2x2 max pooling, bilinear x2 upsampling with align_corners=True (C % 8 == 0) */
int ladi_op_maxpool2(const void* src, int n, int H, int W, int C, void* dst, void* stream);
int ladi_op_upsample2x_bilinear(const void* src, int n, int H, int W, int C, void* dst, void* stream);
int ladi_op_softmax_rows(const float* S, int rows, int cols, float scale, void* P, void* stream);
int ladi_op_small_linear(const void* x, int x_f32, int ldx, const void* W, const void* bias, const void* res, int ldr, int M, int N,
                         int K, int act, int pre_silu, void* out, int out_f32, int ldo, void* stream);
int ladi_op_nchw_to_nhwc(const void* src, int dtype, int n, int C, int H, int W, void* dst, int ld, void* stream);
int ladi_op_nhwc_to_nchw(const void* src, int ld, int n, int C, int H, int W, void* dst, int dtype, void* stream);
/* one scheduler evaluation on device tensors (fused CFG + DDIM/PLMS update), for scheduler parity tests:
 * runs evaluations [0, evals) feeding eps_seq[i] ([2B or B][hw][4] fp16 NHWC per evaluation); latents fp32 [B][hw][4] in/out */
int ladi_op_sched_run(int kind, int steps, const float* alphas_cumprod_host, const void* eps_seq_dev, int evals, int B, int hw,
                      int cfg, float guidance, float* latents_dev, void* stream);
/* the same with per-evaluation step noise (EulerAncestralDiscrete): step_noise_dev fp32 [noise_steps][B][4][hw], noise_steps >= evals */
int ladi_op_sched_run_noise(int kind, int steps, const float* alphas_cumprod_host, const void* eps_seq_dev, int evals, int B, int hw,
                            int cfg, float guidance, float* latents_dev, const float* step_noise_dev, int noise_steps, void* stream);
/* the same with DDIM's eta (ladi_sched_table_eta's table); eta > 0 needs step noise for every evaluation run */
int ladi_op_sched_run_noise_eta(int kind, int steps, const float* alphas_cumprod_host, float eta, const void* eps_seq_dev, int evals, int B,
                                int hw, int cfg, float guidance, float* latents_dev, const float* step_noise_dev, int noise_steps, void* stream);
/* ladi_op_sched_run_noise_eta with a per-evaluation guidance table, guidance rescale phi and a row stride: eps_seq_dev holds, per evaluation,
 * 2B rows [uncond ; cond] of hw pixels, ld_eps halves apart (a multiple of 4; lanes 4.. are never read).  An evaluation whose
 * guidance_tab_host[i] is <= 1 is cond-only and reads rows B..2B-1 alone.  phi in [0, 1] acts on the other evaluations (ladi_op_cfg_stats). */
int ladi_op_sched_run_guided(int kind, int steps, const float* alphas_cumprod_host, float eta, const void* eps_seq_dev, int ld_eps, int evals,
                             int B, int hw, const float* guidance_tab_host, float phi, float* latents_dev, const float* step_noise_dev,
                             int noise_steps, void* stream);
/* ladi_op_sched_run_guided with the latent blend of ladi_tryon_set_preserve: keep_x0_dev / keep_noise_dev fp32 pixel-major [B][hw][4] (16-byte
 * aligned), keep_mask_dev fp32 [B][hw] (non-zero = keep), the coefficients of ladi_sched_keep_coeffs(kind, steps, .., 0) */
int ladi_op_sched_run_keep(int kind, int steps, const float* alphas_cumprod_host, float eta, const void* eps_seq_dev, int ld_eps, int evals, int B,
                           int hw, const float* guidance_tab_host, float phi, float* latents_dev, const float* step_noise_dev, int noise_steps,
                           const float* keep_x0_dev, const float* keep_noise_dev, const float* keep_mask_dev, void* stream);
/* the guidance-rescale statistics kernel on its own: eps_dev [2B][hw] rows of 4 fp16 channels, ld_eps halves apart, uncond half first ->
 * factor_dev[b] = phi * std(cond_b) / std(u_b + guidance (c_b - u_b)) + (1 - phi), fp32 [B].  Bit-reproducible from call to call. */
int ladi_op_cfg_stats(const void* eps_dev, int ld_eps, int B, int hw, float guidance, float phi, float* factor_dev, void* stream);
/* ladi_op_sched_run_guided with perturbed-attention guidance (ladi_tryon_set_pag): pag_tab_host[i] = s_i >= 0 (required), cfg != 0 =
 * CFG-shaped.  eps_seq_dev holds, per evaluation, 3B rows [uncond ; cond ; perturbed] with cfg, 2B rows [cond ; perturbed] without (then
 * guidance_tab_host may be NULL and phi is ignored).  e = u + g (c - u) + s (c - p), or c + s (c - p) without cfg and in a cond-only
 * evaluation, which reads c and p alone; an evaluation with s_i == 0 never reads its perturbed rows.  A table of zeros gives
 * ladi_op_sched_run_guided's latents bit for bit. */
int ladi_op_sched_run_pag(int kind, int steps, const float* alphas_cumprod_host, float eta, const void* eps_seq_dev, int ld_eps, int evals, int B,
                          int hw, int cfg, const float* guidance_tab_host, const float* pag_tab_host, float phi, float* latents_dev,
                          const float* step_noise_dev, int noise_steps, void* stream);
/* ladi_op_cfg_stats with the perturbed rows: eps_dev [3B][hw], the guided prediction is u + guidance (c - u) + pag_scale (c - p).
 * pag_scale == 0 reads the first 2B rows alone and is ladi_op_cfg_stats bit for bit; a negative or non-finite one is an error. */
int ladi_op_cfg_stats_pag(const void* eps_dev, int ld_eps, int B, int hw, float guidance, float pag_scale, float phi, float* factor_dev,
                          void* stream);
/* the identity attention map of PAG on its own: o[row][0:C] = v[row][0:C] for `rows` rows, fp16, row strides ldv / ldo halves (v: the V
 * third of a fused QKV buffer), 16-byte vectors.  C and both strides multiples of 8, strides >= C, both bases 16-byte aligned, else an
 * error with a message and nothing is launched.  Columns [C, ld) are never touched. */
int ladi_op_pag_identity(const void* v_dev, int ldv, void* o_dev, int ldo, long long rows, int C, void* stream);
/* the kernels of self-attention guidance on their own (csrc/sag.hip).
 * ladi_op_sag_map: q, k fp16 with sample s, token t, head h at base + s * sq + t * ld + h * 64 (strides in halves, multiples of 8, row strides
 *   >= 64 * heads, bases 16-byte aligned), any T >= 1 and heads >= 1 -> s_out_dev fp32 [n][T], m_out_dev bytes [n][T] as above.  Allocates
 *   its scratch and synchronises `stream`.  Two calls give the same bits.
 * ladi_op_sag_degrade: latents_dev fp32 [B][h * w][4], eps_dev fp16 [B][h * w][ld_eps] (the base prediction, channels 0..3), mask_dev bytes
 *   [B][hm][wm] -> channels 0..3 of dst_rows_dev fp16 [B][h * w][ld_in] = fp16(in_scale * xd) as under ladi_tryon_set_sag, with the
 *   coefficients given.  src_rows_dev non-NULL and another pointer than dst_rows_dev: its channels [4, copy_end) are copied too (copy_end a
 *   multiple of 4, <= ld_in); else no other channel is touched.  Latents under 5 x 5 are an error.  Synchronises `stream`.
 * ladi_op_cfg_stats_sag: ladi_op_cfg_stats with eps_dev [3B][hw], rows [2B, 3B) the degraded input's prediction d: the guided prediction is
 *   u + guidance (c - u) + sag_scale (u - d).  sag_scale == 0 reads the first 2B rows alone and is ladi_op_cfg_stats bit for bit.
 * ladi_op_sched_run_sag: ladi_op_sched_run_pag's layout with d in the third group of every evaluation and ONE scale: e = u + g (c - u) +
 *   s (u - d) with cfg, c + s (c - d) without and in a cond-only evaluation; phi acts on the whole sum of a CFG evaluation.  s == 0 never
 *   reads the third group and gives ladi_op_sched_run_guided's latents bit for bit. */
int ladi_op_sag_map(const void* q_dev, int ldq, long long sq, const void* k_dev, int ldk, long long sk, int n, int T, int heads, float* s_out_dev,
                    unsigned char* m_out_dev, void* stream);
int ladi_op_sag_degrade(const float* latents_dev, const void* eps_dev, int ld_eps, const unsigned char* mask_dev, int B, int h, int w, int hm,
                        int wm, float sqrt_a, float sqrt_1ma, float in_scale, const void* src_rows_dev, void* dst_rows_dev, int ld_in,
                        int copy_end, void* stream);
int ladi_op_cfg_stats_sag(const void* eps_dev, int ld_eps, int B, int hw, float guidance, float sag_scale, float phi, float* factor_dev,
                          void* stream);
int ladi_op_sched_run_sag(int kind, int steps, const float* alphas_cumprod_host, float eta, const void* eps_seq_dev, int ld_eps, int evals, int B,
                          int hw, int cfg, const float* guidance_tab_host, float sag_scale, float phi, float* latents_dev,
                          const float* step_noise_dev, int noise_steps, void* stream);
/* pipeline pre-processing kernels, one entry point per kernel so each can be checked on its own:
 * prepare_mask_and_masked_image (diffusers tensor branch; tryon_pipe.py:630): mask binarised at 0.5 -> mask_bin_dev fp16 [B,H,W];
 *   masked_image_dev NHWC fp16 [B,H,W,ld] (3 valid channels, the rest zero) = image * (mask < 0.5) */
int ladi_op_prepare_mask(const void* image_dev, const void* mask_dev, int dtype, int B, int H, int W, void* masked_image_dev, int ld,
                         void* mask_bin_dev, void* stream);
/* F.interpolate(mask, size=(H/s, W/s)) (nearest; prepare_mask_latents tryon_pipe.py:424-427, mask_features data_utils.py:11) on fp16 [B,H,W] */
int ladi_op_mask_down(const void* mask_dev, int B, int H, int W, int s, void* out_dev, void* stream);
/* F.interpolate(pose_map, size=(H/8, W/8), mode="bilinear") (tryon_pipe.py:632-634): NCHW in (dtype) -> NHWC fp16 [B, H/8 * W/8, C] */
int ladi_op_pose_down8(const void* pose_dev, int dtype, int B, int C, int H, int W, void* out_dev, void* stream);
/* scaling_factor * DiagonalGaussianDistribution(moments).sample() (vae.py:329-348; tryon_pipe.py:640,647) with the generator draw passed in:
 * moments NHWC fp16 [B, hw, ldm] (8 channels: mean | logvar), noise fp32 NCHW [B,4,h,w] -> latents fp32 [B, hw, 4] */
int ladi_op_posterior_sample(const void* moments_dev, int ldm, const float* noise_dev, int B, int hw, float scaling, float* lat_dev,
                             void* stream);
/* 31-channel UNet input assembly (tryon_pipe.py:702-729): [latents(4) | mask(1) | masked-image latents(4) | pose(P) | cloth latents(4)],
 * CFG batch order [uncond(B); cond(B)] with zero pose / cloth in the uncond half; unet_in NHWC fp16 [(cfg ? 2B : B), hw, ld] */
int ladi_op_assemble_input(void* unet_in_dev, int ld, int B, int hw, int cfg, const float* latents_dev, const void* mask_lat_dev,
                           const float* masked_lat_dev, const void* pose_dev, int pose_channels, const float* cloth_lat_dev, void* stream);
/* ---- helper kernels on their own (tests/test_gpu_helpers.py): one entry point per launcher, device pointers, the launcher's return code.
 * Row strides are in elements; columns [C, ld) of a strided row are neither read nor written unless a line below says they are zeroed.
 * One query per (sample, head) -- the inversion adapter's pooling attention: q [n][ldq], k / v rows [n][Nk][ld] with sample strides sk / sv,
 * head h at column h * d of every row, any d <= 128 (d > 128: -1), out [n][ldo] */
int ladi_op_attention_single_query(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int n, int heads,
                                   int d, int Nk, long long sk, long long sv, float scale, void* stream);
/* the image-prompt term of a cross-attention on its own (csrc/ip_adapter.hip), in place on o:
 *   o[s][t][h*64 + d] = fp16(float(o[s][t][h*64 + d]) + scale * sum_j softmax_j(0.125 <q[s][t][h], k[s][j][h]>) v[s][j][h*64 + d]),  j < N
 * fp32 with the row maximum subtracted, one rounding per element; head dimension 64.  Row strides ldq / ldk / ldv / ldo and per-sample
 * strides sq / sk / sv / so in elements (the kv_cache layout: k = kv, v = kv + C, ldk = ldv = 2C, sk = sv = N * 2C).  Rows t >= T and columns
 * >= heads * 64 are never touched.  -1 with a message, nothing launched: N outside [1, 64], n / heads / T < 1, a null pointer, a row stride
 * that is not a multiple of 8 or below heads * 64, a per-sample stride that is not a multiple of 8, a base that is not 16-byte aligned */
int ladi_op_ip_attn_add(const void* q, int ldq, long long sq, const void* k, int ldk, long long sk, const void* v, int ldv, long long sv, void* o,
                        int ldo, long long so, int n, int heads, int T, int N, float scale, void* stream);
/* fp32 path of the warping module (TPS network and refinement UNet called with fp32 tensors): NHWC fp32 activations, fp32 weights
 * [Q][ksize * ksize * (C0 + C1)] tap-major / channel-minor (row stride ldw, 0 = K), out = act(conv + bias) (act: 0 none, 1 SiLU, 4 ReLU, 5 tanh).
 * batch > 1 runs `batch` problems bs_src0 / bs_w / bs_out elements apart (the correlation: the weight operand is a feature map).
 * Refused without a launch: -1 ksize outside 1..4, C0 / C1 not multiples of 8, ld0 / ld1 not multiples of 4, P or Q <= 0; -3 K != ksize^2 (C0 + C1)
 * or ldw not a multiple of 4; -4 src0 / src1 / W / out not 16-byte aligned; -5 ld0 < C0 or ld1 < C1; -6 batch > 1 with a second source (it has
 * no batch stride); -7 batch > 1 with bs_src0 or bs_w, or -- when ldo % 4 == 0, the vector store -- bs_out, not a multiple of 4 */
typedef struct {
    const float* src0; const float* src1; int C0, C1, ld0, ld1, Hs, Ws, Ho, Wo, P, ksize, stride, pad;
    const float* W; int Q, K, ldw; long long bs_src0, bs_w, bs_out; const float* bias; int act; float* out; int ldo;
} ladi_conv_f32_desc;
int ladi_op_conv_f32(const ladi_conv_f32_desc* d, int batch, void* stream);
/* NCHW (dtype 0 fp32 / 1 fp16) <-> NHWC fp32 [n][H W][ld]; to NHWC zeroes channels [C, ld) */
int ladi_op_nchw_to_nhwc_f32(const void* src, int dtype, int n, int C, int H, int W, float* dst, int ld, void* stream);
int ladi_op_nhwc_to_nchw_f32(const float* src, int ld, int n, int C, int H, int W, void* dst, int dtype, void* stream);
/* x = x * scale[c] + shift[c] in place; x /= sqrt(sum_c x^2 + 1e-6) in place; dst[i][:] = src[rows[i]][:] (dense rows of H floats) */
int ladi_op_channel_affine_f32(float* x, int ld, long long n_pix, int C, const float* scale, const float* shift, void* stream);
int ladi_op_l2norm_rows_f32(float* x, int ld, int rows, int C, void* stream);
int ladi_op_gather_rows_f32(const float* src, const int* rows, int n, int H, float* dst, void* stream);
int ladi_op_maxpool2_f32(const float* src, int lds, int n, int H, int W, int C, float* dst, int ldd, void* stream);
int ladi_op_upsample2x_bilinear_f32(const float* src, int lds, int n, int H, int W, int C, float* dst, int ldd, void* stream);
/* out[m][n] = act(sum_k x[m][k] W[n][k] + b[n]), everything fp32, W dense [N][K] */
int ladi_op_linear_f32(const float* x, int ldx, const float* W, const float* b, int M, int N, int K, int act, float* out, int ldo, void* stream);
/* the fp16 forms of the TPS network (C, ldx, ldy multiples of 8; channel_affine may run in place) */
int ladi_op_channel_affine(const void* x, int ldx, long long n_pix, int C, const float* scale, const float* shift, void* y, int ldy, void* stream);
int ladi_op_l2norm_rows(const void* x, int ldx, int rows, int C, void* y, int ldy, void* stream);
int ladi_op_gather_rows(const void* src, const int* rows, int n, int H, void* dst, void* stream);
/* TPSGridGen: coor [B][N][2], inv [(N + 3)^2], ctrl [N][2] (fp32) -> grid fp32 [B][H][W][2]; 1 <= N <= 32 and H, W >= 2, else -1 */
int ladi_op_tps_grid(const float* coor, const float* inv, const float* ctrl, int N, int B, int H, int W, float* grid, void* stream);
/* CLIP text front end on device ids [B][T]: first[b] = position of the first `vstar` id (-1: none, or use_words == 0), eot[b] = b T + argmax
 * (first maximum); out [B][T][H] = (token | spliced pseudo-word) + position embedding, ids clamped to [0, vocab), wemb [B][nv][H] or NULL */
int ladi_op_text_meta(const int* ids, int B, int T, int vstar, int use_words, int* first, int* eot, void* stream);
int ladi_op_text_embed(const int* ids, const int* first, int nv, const void* tok, const void* pos, const void* wemb, int B, int T, int H,
                       int vocab, void* out, void* stream);
/* ViT patch rows: px [B][3][S][S] (dtype) -> out fp16 [B][1 + (S / ps)^2][KP], row 0 and columns >= 3 ps^2 zero */
int ladi_op_patchify(const void* px, int dtype, int B, int S, int ps, int KP, void* out, void* stream);
/* glue of the denoising loop and the decoder */
int ladi_op_timestep_embedding(const float* t, int count, int dim, float* out, void* stream);     /* [cos | sin], fp32 [count][dim] */
int ladi_op_image_post(const void* src, int ld, int n_pix, void* dst, int dst_u8, void* stream);  /* clamp(x / 2 + 0.5, 0, 1): fp32 or round(255 v) u8, [n_pix][3] */
/* preserve-unmasked kernels on their own.  mask_pool8: out fp32 [B][H/8][W/8] = F.max_pool2d(mask, 8) of the binarised fp16 mask [B][H][W]
 * (16-byte aligned; H, W multiples of 8), with invert 1 - that (the keep mask).  mask_feather: out fp32 [B][H][W] = the separable Gaussian blur
 * of the fp16 mask (sigma in (0, 32], radius ceil(3 sigma) = the return value, weights normalised in double, replicate border, rows into tmp
 * fp32 [B][H][W] then columns).  image_composite: dst [B * HW][3] (fp32 or, dst_u8, round(255 v)) = M g + (1 - M) p from the decoded NHWC fp16
 * tensor (row stride ld, a multiple of 4), the NCHW image (dtype) and the mask [B][HW] (fp16, or fp32 with mask_f32); HW a multiple of 4 */
int ladi_op_mask_pool8(const void* mask_bin, int B, int H, int W, int invert, float* out, void* stream);
int ladi_op_mask_feather(const void* mask_bin, int B, int H, int W, float sigma, float* tmp, float* out, void* stream);
int ladi_op_image_composite(const void* decoded, int ld, const void* image, int dtype, const void* mask, int mask_f32, int B, int HW, void* dst,
                            int dst_u8, void* stream);
int ladi_op_post_quant(const float* lat, const float* pq, float inv_sf, int n, void* dst, int ld, void* stream);   /* pq [16 w | 4 b] or NULL; channels [4, ld) zero */
int ladi_op_lat_nchw_to_pix(const float* src, int B, int hw, float scale, float* dst, void* stream);
int ladi_op_lat_pix_to_nchw(const float* src, int B, int hw, float* dst, void* stream);
/* start latents (ladi_tryon_set_init): out fp32 [B][h*w][4] = k_x * resample(init fp32 [B][4][hs][ws]) + k_n * noise fp32 [B][4][h][w]; bilinear,
 * source coordinate max((o + 0.5) * in / out - 0.5, 0), no antialias; equal sizes: k_x * init + k_n * noise without interpolation arithmetic.
 * noise may be NULL when k_n == 0 (it is never read then).  A null init / out, a size < 1 or a null noise with k_n != 0 is an error. */
int ladi_op_init_latents(const float* init, int hs, int ws, const float* noise, int B, int h, int w, float k_x, float k_n, float* out, void* stream);
/* src fp32 NCHW [B][4][hw] -> latents [B][hw][4] and channels 0-3 of unet_in rows ([B], with cfg [2B]; ld_in >= 4, a multiple of 4) = fp16(x in_scale) */
int ladi_op_latents_import(const float* src, int B, int hw, float* latents, void* unet_in, int ld_in, int cfg, float in_scale, void* stream);
int ladi_op_scale_h16(const void* src, int lds, void* dst, int ldd, long long n_pix, int C, float s, void* stream);
int ladi_op_fill_f32(float* p, long long n, float v, void* stream);
/* one FreeU site.  hidden NHWC fp16 [n][H][W] rows of ld_h halves: channels [0, C_h / 2) become fp16(float(x) * b) in place, every other
 * half of a row keeps its bits.  skip NHWC fp16 (ld_s) -> skip_out NHWC fp16 (ld_d; skip_out == skip allowed): each (sample, channel) plane
 * becomes x + (s - 1) lp, lp the part of x at the frequencies {0, -1 mod H} x {0, -1 mod W} (fourier_filter, threshold 1) -- fp32 sums in a
 * fixed order (two launches are bit-equal), one rounding; halves outside [0, C_s) of a skip_out row are not written.  hidden == NULL or
 * skip == NULL does only the other half.  Any H, W >= 1; C_h % 16 == 0, C_s % 8 == 0, every ld a multiple of 8 and >= C, 16-byte aligned
 * pointers: anything else is refused with a message and nothing is launched. */
int ladi_op_freeu(void* hidden, int ld_h, int C_h, float b, const void* skip, int ld_s, int C_s, float s, void* skip_out, int ld_d, int n, int H,
                  int W, void* stream);
/* one LoRA merge: rows [row0, row0 + rows) of the packed fp16 weight W (rows of `pitch` halves, each [taps][cin_pad]) become
 *   fp16(float(base) + sum_a scale[a] * sum_r up[a][o][r] * down[a][r][t][i])      for the channels i < cin of every tap
 * from the same rows of `base` (same layout, read only, not W itself).  up[a] fp32 [rows][rank[a]], down[a] fp32 [rank[a]][taps][cin].
 * geglu_half = 0: source row o is row row0 + o; geglu_half = rows / 2: the GEGLU interleave (o < half -> row0 + 64 (o / 32) + o % 32, half + o
 * -> the same + 32; half a multiple of 32, row0 of 64).  fp32 sums in a fixed order (ascending r, adapters in call order), one rounding: two
 * launches are bit-equal; n_adapters = 0 or a delta of exactly zero copies the base's bits.  Channels [cin, cin_pad) and all other rows
 * keep their bits.  nonfinite (device, may be NULL) += the number of results outside the fp16 range.  cin_pad a multiple of 64 and >= cin,
 * pitch a multiple of 8 and >= taps * cin_pad, 16-byte aligned base / W, at most 8 adapters of rank 1 .. 256, finite scales: anything else is
 * refused with a message and nothing is launched. */
int ladi_op_lora_merge(const void* base, void* W, long long pitch, int cin, int cin_pad, int taps, int row0, int rows, int geglu_half,
                       int n_adapters, const float* const* up, const float* const* down, const int* rank, const float* scale,
                       unsigned* nonfinite, void* stream);

/* ---- Token merging (DESIGN.md "Token merging"; tomesd.apply_patch, bipartite_soft_matching_random2d) ----
 * In the transformer blocks of the first max_downsample levels of the UNet (1: the full-resolution level, down_blocks.0 and up_blocks.3; 2:
 * also the half-resolution level) the selected sub-layers run over T - r rows, r = min(int(T * ratio), Ns).  The T = h w tokens of a block
 * are split into one dst token per full sy x sx cell -- at in-cell offset 0, or with use_rand at splitmix64(seed * 2^32 + cell) mod (sx sy),
 * computed on the host, the same for every block of a level and every evaluation (tomesd redraws per block and evaluation) -- and Ns src
 * tokens (every other token, leftover rows and columns of an odd side included).  Every src is matched to the dst with the largest cosine
 * similarity of the block's token input (the output of proj_in; fp16 unit rows, fp32 accumulation; ties to the lower dst), the r src with
 * the largest score (ties to the lower src, NaN as -inf) are averaged into their dst (fp32, ascending src order, one rounding), and a merged
 * sub-layer is x = u(f(m(norm x))) + x over the rows [unmerged src, ascending ; dst]: attn1 with merge_attn, attn2 (its queries, and the
 * IP-Adapter image term's) with merge_crossattn, the feed-forward with merge_mlp, one plan per block.  Sticky per UNet, off by default;
 * holds for the stand-alone forwards, the cached forms and the fused loop (whose graphs are keyed on it).  cfg NULL or ratio 0 switches it
 * off: the forward then launches exactly the plain forward.  A block whose level gives r = 0 runs the plain path.
 * Refused with a message (-1, nothing changed): ratio outside [0, 1) or not finite, sx or sy other than 2, max_downsample other than 1 or 2,
 * all three merge flags off with ratio > 0.  A forward refuses (with a message) a level of more than 4096 dst tokens or a block width that
 * is no multiple of 64 or above 960, and perturbed (PAG) samples in a block that merges. */
typedef struct {
    double ratio;
    int max_downsample, sx, sy, use_rand;
    unsigned seed;
    int merge_attn, merge_crossattn, merge_mlp;
} ladi_tome_config;
int ladi_tome_config_check(const ladi_tome_config* cfg);                    /* host only: 0, or -1 with the refusal as the last error */
int ladi_unet_set_token_merging(ladi_unet* u, const ladi_tome_config* cfg);
int ladi_unet_token_merging(const ladi_unet* u, ladi_tome_config* cfg_out);  /* 1 on, 0 off (cfg_out then holds the defaults), -1 null handle */
/* the merged transformer blocks, in execution order; blocks_out (may be NULL) receives their indices in PAG's block numbering */
int ladi_unet_tome_block_count(const ladi_unet* u, int* blocks_out, int cap);
/* out_row of merged block `block` (0 .. count - 1) as the last forward left it: n * T ints for the n samples of the context batch, entry
 * [s][p] the row of the merged sequence that token p of sample s reads (its own row for an unmerged src, Nu + j for dst j and every src
 * merged into it) -- also what a visualisation of the merges needs.  Synchronises the device.  Returns n * T (copied when cap is at least
 * that), 0 when the block merges nothing at the last size, < 0 on error. */
int ladi_unet_tome_read_plan(ladi_unet* u, int block, int* out_row_host, int cap);
/* host only: the partition of h x w tokens.  Returns Nd = (h / sy) * (w / sx) and, with both pointers given and cap >= max(Nd, h w - Nd),
 * the token positions of the src (h w - Nd of them) and of the dst tokens, each ascending; -1 on a refusal. */
int ladi_tome_tables(int h, int w, int sx, int sy, int use_rand, unsigned seed, int* src_pos, int* dst_pos, int cap);
int ladi_tome_merge_count(int T, int Ns, double ratio);                     /* host only: r, or -1 for a ratio outside [0, 1) */
/* the kernels on their own (csrc/tome.hip).  Tables and plans are device int32; n samples of T = Ns + Nd tokens, rows of C halves.
 * match: prep + match over the metric x (row stride ld, per-sample stride sx elements): score[n][Ns] fp32, node[n][Ns]; C % 64 == 0, C <= 960;
 *   workspace of ladi_op_tome_match_workspace_bytes(n, Ns, Nd, C) bytes, 16-byte aligned.
 * plan: out_row[n][T] and plan[n][ladi_op_tome_plan_ints(Ns, Nd, r)] = seg_off (Nd + 1) | unm_pos (Ns - r) | seg_src (r) | scratch (r);
 *   1 <= r <= Ns, Nd <= 4096.
 * merge: y[n][T - r] from x with such a plan (r = 0 allowed: a permutation); unmerge_add: out[s][p] = fp16(y[s][out_row[s][p]] + res[s][p]).
 * C % 8 == 0, strides multiples of 8 and >= C, 16-byte aligned bases: anything else is refused with a message and nothing is launched. */
long long ladi_op_tome_match_workspace_bytes(int n, int Ns, int Nd, int C);
long long ladi_op_tome_plan_ints(int Ns, int Nd, int r);
int ladi_op_tome_match(const void* x, int ld, long long sx, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int C,
                       void* workspace, float* score, int* node, void* stream);
int ladi_op_tome_plan(const float* score, const int* node, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int r,
                      int* out_row, int* plan, void* stream);
int ladi_op_tome_merge(const void* x, int ldx, long long sx, const int* dst_pos, const int* plan, int n, int T, int Ns, int Nd, int r, int C,
                       void* y, int ldy, long long sy, void* stream);
int ladi_op_tome_unmerge_add(const void* y, int ldy, long long sy, const void* res, int ldr, long long sr, const int* out_row, int n, int T,
                             int Tm, int C, void* out, int ldo, long long so, void* stream);

/* ---- fp16 range probe (opt-in; with no probe attached nothing changes: same launches, same captured graph, same bits) ----
 * A probe records, for every named activation of the modules it is attached to, the largest finite |x| and the number of inf / NaN
 * elements the fp16 tensor held (one extra read of the tensor per point; values accumulate -- max / sum -- until ladi_probe_reset).
 * Points are named by the diffusers key prefix of the module that produced the tensor:
 *   UNet:    conv_in, down_blocks.I.resnets.J, down_blocks.I.attentions.J, down_blocks.I.downsamplers.0, mid_block.resnets.0,
 *            mid_block.attentions.0, mid_block.resnets.1, up_blocks.I.resnets.J, up_blocks.I.attentions.J, up_blocks.I.upsamplers.0, conv_out
 *   VAE:     encoder.conv_in, encoder.down_blocks.I, encoder.mid_block, quant_conv (the moments); post_quant_conv, decoder.mid_block,
 *            decoder.up_blocks.I, decoder.conv_out -- the decoder's stream points are what the stream holds (an EMASC skip that the
 *            producing kernel folds in included) and are reported at their TRUE scale under a range shift
 *   EMASC:   emasc.I
 * A name gets its slot the first time a run meets it, so slot order is execution order.  One probe may be attached to several modules
 * (a second UNet on the same probe would share the first one's names).  A probe must outlive its attachments: detach (attach NULL)
 * or destroy the modules before ladi_probe_destroy, which otherwise destroys nothing and leaves a message for ladi_last_error.  Inside
 * ladi_tryon_run the attached probes are zeroed at the start of the run and the UNet slots accumulate over all evaluations. */
typedef struct ladi_probe ladi_probe;
ladi_probe* ladi_probe_create(int max_points);
void ladi_probe_destroy(ladi_probe* p);
int ladi_unet_attach_probe(ladi_unet* u, ladi_probe* p);     /* NULL detaches; same for vae / emasc */
int ladi_vae_attach_probe(ladi_vae* v, ladi_probe* p);
int ladi_emasc_attach_probe(ladi_emasc* e, ladi_probe* p);
int ladi_probe_count(const ladi_probe* p);                   /* registered points, -1 on a null handle */
const char* ladi_probe_name(const ladi_probe* p, int i);     /* NULL when out of range; valid until the probe is destroyed */
/* absmax_out[i] / nonfinite_out[i] (host; either may be NULL) of the first min(count, cap) points; returns the point count, < 0 on error.
 * Synchronises `stream`. */
int ladi_probe_read(ladi_probe* p, float* absmax_out, unsigned* nonfinite_out, int cap, void* stream);
/* rank_out[i] (host) = the rank in TIME (1, 2, ...) at which point i first held an inf / NaN since the last reset, 0 = never.  Point
 * order is the order of one forward; inside the denoising loop a NaN of one evaluation comes back into the first points of the next, so
 * "which layer left the range first" is the point of rank 1.  Returns the point count, < 0 on error.  Synchronises `stream`. */
int ladi_probe_read_rank(ladi_probe* p, unsigned* rank_out, int cap, void* stream);
int ladi_probe_reset(ladi_probe* p, void* stream);           /* zero every slot and rank, asynchronous on `stream` */
/* the probe kernel on its own: over the C valid lanes of each of `rows` rows of an fp16 view (row stride ld >= C halves; lanes C..ld-1 are
 * never read; any C, ld and 2-byte alignment): *absmax_dev = max(*absmax_dev, max |x| over finite x) and *nonfinite_dev += #(inf / NaN).
 * Both words are device memory the caller zeroes; *absmax_dev must be a non-negative float. */
int ladi_op_absmax(const void* x, int rows, int C, int ld, float* absmax_dev, unsigned* nonfinite_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
