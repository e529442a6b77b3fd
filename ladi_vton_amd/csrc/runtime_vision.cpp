// CLIP ViT-H/14 vision encoder: native counterpart of the transformers 4.27.3 CLIPVisionTransformer the reference calls at
// src/inference.py:269-273 (`vision_encoder(pixel_values).last_hidden_state`, consumed by the inversion adapter at :276).
// Patch embedding = patch-row gather + one GEMM whose epilogue adds the (class-token-augmented) position embeddings, pre_layrnorm,
// 32 pre-LN blocks (fused QKV GEMM, d = 80 MFMA attention, out-proj + residual, gelu MLP).  Once per batch, outside the denoising loop.
#include "runtime.h"
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>

namespace ladi {

void VisionEncoder::load(const VisionCfg& c, const WeightStore& ws) {
    cfg = c;
    const int H = c.hidden, d = H / c.heads;
    if (H % 32 || c.heads * d != H || !(d == 64 || d == 80 || d == 96 || d == 128)) throw std::runtime_error("vision encoder: head dim must be 64/80/96/128");
    if (c.image % c.patch) throw std::runtime_error("vision encoder: image size must be a multiple of the patch size");
    const std::string pre = ws.has("vision_model.embeddings.class_embedding") ? "vision_model." : "";
    const HostTensor& pw = ws.get(pre + "embeddings.patch_embedding.weight");
    const HostTensor& ce = ws.get(pre + "embeddings.class_embedding");
    const HostTensor& pe = ws.get(pre + "embeddings.position_embedding.weight");
    const int nk = 3 * c.patch * c.patch, kp = (nk + 63) / 64 * 64, T = tokens();
    if (pw.numel() != (size_t)H * nk || ce.numel() != (size_t)H || pe.numel() != (size_t)T * H) throw std::runtime_error("vision encoder: embedding shapes");
    std::vector<float> w((size_t)H * kp, 0.f);
    for (int q = 0; q < H; ++q) std::memcpy(&w[(size_t)q * kp], &pw.data[(size_t)q * nk], (size_t)nk * sizeof(float));
    patch.w = pool.upload_h16(w); patch.b = nullptr; patch.cin = nk; patch.cin_pad = kp; patch.cout = H; patch.k = 1;
    std::vector<float> pc(pe.data);
    for (int i = 0; i < H; ++i) pc[i] += ce.data[i];          // the class token sits in row 0 (its patch row is zero)
    posc = pool.upload_h16(pc);
    pre_ln = load_norm(pool, ws, pre + "pre_layrnorm");      // (sic: the key is misspelled upstream)
    post_ln = load_norm(pool, ws, pre + "post_layernorm");
    layers = load_clip_layers(pool, ws, pre + "encoder.layers.", c.layers);
    if (ws.has("visual_projection.weight")) {                // CLIPVisionModelWithProjection: Linear(hidden -> projection_dim), no bias
        const HostTensor& vp = ws.get("visual_projection.weight");
        if (vp.shape.size() != 2 || vp.shape[1] != H || vp.shape[0] < 1)
            throw std::runtime_error("vision encoder: visual_projection.weight is not [projection_dim, " + std::to_string(H) + "]");
        if (ws.has("visual_projection.bias")) throw std::runtime_error("vision encoder: visual_projection has no bias");
        vproj = pool.upload_h16(vp.data);
        proj_dim = (int)vp.shape[0];
    }
}

int VisionEncoder::forward(const void* pixels, int in_f32, int B, h16* out_hidden, h16* out_pooled, hipStream_t st) {
    return forward_ex(pixels, in_f32, B, out_hidden, out_pooled, nullptr, nullptr, st);
}

int VisionEncoder::forward_ex(const void* pixels, int in_f32, int B, h16* out_hidden, h16* out_pooled, h16* out_pen, h16* out_embeds,
                              hipStream_t st) {
    if (B <= 0) { set_error("vision encoder: bad batch"); return -1; }
    if (out_embeds && !vproj) {
        set_error("vision encoder: image_embeds asked for, but the weights hold no visual_projection.weight");
        return -1;
    }
    const int H = cfg.hidden, T = tokens(), nl = (int)layers.size();
    const bool need_pooled = out_pooled || out_embeds;
    if (!out_hidden && !need_pooled && !out_pen) return 0;
    run_planned(arena, st, [&](Ctx& c) {
        Act xa = c.new_act(B, T, 1, H), xb = c.new_act(B, T, 1, H);   // residual stream, ping-pong
        // every call runs the whole encoder: an output the caller did not ask for lives in the arena
        h16* hidden = out_hidden ? out_hidden : c.alloc_h16((size_t)B * T * H);
        h16* pooled = out_pooled ? out_pooled : (need_pooled ? c.alloc_h16((size_t)B * H) : nullptr);
        Act last = xa; last.p = hidden; last.ld = H;          // the last block writes straight into the caller's buffer
        Act pen = xa; pen.p = out_pen; pen.ld = H;            // ... and so does the producer of the last block's input
        Act* cur = &xa; Act* nxt = &xb;
        if (out_pen && nl == 1) cur = &pen;
        {   // embeddings: patch rows -> GEMM (+ position / class embeddings as the residual, shared by every image) -> pre_layrnorm
            const size_t mk = c.ar->mark();
            Act pr = c.new_act(B, T, 1, patch.cin_pad);
            Act emb = c.new_act(B, T, 1, H);
            if (!c.dry()) {
                c.check(ladi_launch_patchify(pixels, in_f32, B, cfg.image, cfg.patch, patch.cin_pad, pr.p, st), "patchify");
                IGemmArgs g;
                std::memset(&g, 0, sizeof(g));
                g.src0 = pr.p; g.C0 = pr.c; g.ld0 = pr.ld; g.Hs = T; g.Ws = 1; g.Ho = T; g.Wo = 1; g.P = T;
                g.ksize = 1; g.stride = 1; g.pad = 0; g.W = patch.w; g.Q = H; g.K = patch.K();
                g.bs_src0 = (long long)T * pr.ld; g.bs_w = 0; g.bs_out = (long long)T * emb.ld; g.bs_res = 0;
                g.act = LADI_ACT_NONE; g.out_scale = 1.f; g.res0 = posc; g.ldr0 = H; g.out = emb.p; g.ldo = emb.ld;
                c.check(ladi_launch_igemm(g, B, 0, st), "patch embedding");
                c.check(ladi_launch_layernorm(emb.p, emb.ld, pre_ln.g, pre_ln.b, cfg.ln_eps, B * T, H, cur->p, cur->ld, st), "pre_layrnorm");
            }
            c.ar->release(mk);
        }
        for (int i = 0; i < nl; ++i) {
            Act* dst = i == nl - 1 ? &last : (i == nl - 2 && out_pen) ? &pen : nxt;
            clip_layer(c, layers[i], *cur, *dst, cfg.heads, false, cfg.ln_eps);
            if (dst == nxt) std::swap(cur, nxt);
            else cur = dst;
        }
        if (!c.dry() && need_pooled)
            c.check(ladi_launch_layernorm(hidden, T * H, post_ln.g, post_ln.b, cfg.ln_eps, B, H, pooled, H, st), "post_layernorm");
        if (!c.dry() && out_embeds)
            c.check(ladi_launch_small_linear(pooled, 0, H, vproj, nullptr, nullptr, 0, B, proj_dim, H, LADI_ACT_NONE, 0, out_embeds, 0, proj_dim, st),
                    "visual_projection");
    });
    return 0;
}

}  // namespace ladi
