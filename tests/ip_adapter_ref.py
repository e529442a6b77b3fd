"""Reference for the IP-Adapter image prompt (diffusers IPAdapterAttnProcessor2_0 with the plain ImageProjection): the yardstick
tests/test_cpu_ip_adapter.py and tests/test_gpu_ip_adapter.py compare the library with.  The forward is tests/pag_ref.py's composition of
oracle.models' block functions, with a transformer2d whose cross-attention has the second, decoupled term
    attn2_out = to_out(attention(q, k_text, v_text) + s_block * attention(q, to_k_ip(tokens), to_v_ip(tokens)))
and the same perturbation of attn1 (PAG), so that PAG + IP has a reference.  Nothing here imports the package under test except its
scheduler mirrors (through tests/pag_ref.py).

    sd_ip     the adapter under the library's keys (ladi_vton_amd.ip_adapter.load_state's output): image_proj.{proj,norm}.{weight,bias} and
              <block>.transformer_blocks.0.attn2.processor.to_{k,v}_ip.weight
    tokens    [n, N, cross_dim]: image_proj(sd_ip, embeds), or anything else (set_ip_tokens)
    scales    one float per transformer block in execution order (pag_ref.block_prefixes)
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from tests import freeu_ref as FU
from tests import guidance_ref as G
from tests import pag_ref as R
from tests import strength_ref as SR

PROC = ".transformer_blocks.0.attn2.processor."


def image_proj(sd_ip, embeds):
    """ImageProjection: LayerNorm(Linear(embeds)) per token, eps 1e-5; embeds [n, E] -> [n, N, cross_dim]"""
    D = sd_ip["image_proj.norm.weight"].numel()
    t = F.linear(embeds, sd_ip["image_proj.proj.weight"], sd_ip["image_proj.proj.bias"]).reshape(embeds.shape[0], -1, D)
    return F.layer_norm(t, (D,), sd_ip["image_proj.norm.weight"], sd_ip["image_proj.norm.bias"], 1e-5)


def transformer2d(sd, p, x, ehs, heads, groups, perturbed_from=None, ip=None):
    """pag_ref.transformer2d with the image term; ip = (sd_ip, tokens, scale of THIS block) or None"""
    if ip is None:
        return R.transformer2d(sd, p, x, ehs, heads, groups, perturbed_from)
    sd_ip, tokens, scale = ip
    n, C, h, w = x.shape
    res = x
    t = M.group_norm(sd, p + ".norm", x, groups, 1e-6).permute(0, 2, 3, 1).reshape(n, h * w, C)
    t = M.linear(sd, p + ".proj_in", t)
    b = p + ".transformer_blocks.0"
    a = M.layer_norm(sd, b + ".norm1", t)
    q, k, v = M.linear(sd, b + ".attn1.to_q", a), M.linear(sd, b + ".attn1.to_k", a), M.linear(sd, b + ".attn1.to_v", a)
    k0 = n if perturbed_from is None else max(0, min(n, perturbed_from))
    o = v.clone()                                     # the identity attention map: O = V
    if k0 > 0:
        o[:k0] = M.attention(q[:k0], k[:k0], v[:k0], heads)
    t = M.linear(sd, b + ".attn1.to_out.0", o) + t
    a = M.layer_norm(sd, b + ".norm2", t)
    q2 = M.linear(sd, b + ".attn2.to_q", a)
    o2 = M.attention(q2, M.linear(sd, b + ".attn2.to_k", ehs), M.linear(sd, b + ".attn2.to_v", ehs), heads)
    o2 = o2 + scale * M.attention(q2, F.linear(tokens, sd_ip[p + PROC + "to_k_ip.weight"]), F.linear(tokens, sd_ip[p + PROC + "to_v_ip.weight"]), heads)
    t = M.linear(sd, b + ".attn2.to_out.0", o2) + t
    a = M.layer_norm(sd, b + ".norm3", t)
    u, g = M.linear(sd, b + ".ff.net.0.proj", a).chunk(2, dim=-1)
    t = M.linear(sd, b + ".ff.net.2", u * F.gelu(g)) + t
    t = M.linear(sd, p + ".proj_out", t)
    return t.reshape(n, h, w, C).permute(0, 3, 1, 2) + res


def unet_forward(sd, cfg, sample, timestep, ehs, layers=(), pag_first=None, freeu=None, ip=None):
    """pag_ref.unet_forward with ip = (sd_ip, tokens [n, N, cross_dim], scales) or None (then pag_ref.unet_forward itself)"""
    if ip is None:
        return R.unet_forward(sd, cfg, sample, timestep, ehs, layers, pag_first, freeu)
    sd_ip, tokens, scales = ip
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G_, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    n = sample.shape[0]
    layers = set(layers)
    index = {b: i for i, b in enumerate(R.block_prefixes(L))}
    assert len(scales) == len(index) and tokens.shape[0] == n

    def xf(p, x, hd):
        s = float(scales[index[p]])
        return transformer2d(sd, p, x, ehs, hd, G_, pag_first if p in layers else None, (sd_ip, tokens, s) if s != 0.0 else None)
    forward_upsample_size = any(s % 8 != 0 for s in sample.shape[-2:])
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = M.conv(sd, "conv_in", sample)
    skips = [x]
    for i in range(4):
        for j in range(L):
            x = M.resnet(sd, "down_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i < 3:
                x = xf("down_blocks.%d.attentions.%d" % (i, j), x, heads[i])
            skips.append(x)
        if i < 3:
            x = M.conv(sd, "down_blocks.%d.downsamplers.0.conv" % i, x, stride=2, padding=1)
            skips.append(x)
    x = M.resnet(sd, "mid_block.resnets.0", x, temb, G_, eps)
    x = xf("mid_block.attentions.0", x, heads[3])
    x = M.resnet(sd, "mid_block.resnets.1", x, temb, G_, eps)
    for i in range(4):
        for j in range(L + 1):
            x, sk = FU.apply_freeu(i, x, skips.pop(), freeu)
            x = torch.cat([x, sk], dim=1)
            x = M.resnet(sd, "up_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i > 0:
                x = xf("up_blocks.%d.attentions.%d" % (i, j), x, heads[3 - i])
        if i < 3:
            if forward_upsample_size:
                x = F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = M.conv(sd, "up_blocks.%d.upsamplers.0.conv" % i, x)
    assert not skips
    return M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G_, eps)))


def make_adapter(cfg, N=4, E=64, seed=0, k_scale=1.0, v_scale=0.5):
    """a random adapter under the library's keys (fp16-representable float32).  Tokens are LayerNorm outputs (unit variance), so the image
    keys and values have the standard deviations k_scale / v_scale per channel: logits of order k_scale |q| / 8 and an image term of order
    v_scale, chosen so that the term is visible in the forward (tests/test_cpu_ip_adapter.py checks the margins)."""
    g = torch.Generator().manual_seed(4200 + seed)
    D = cfg["cross_attention_dim"]
    r = lambda *s: torch.randn(s, generator=g)
    h = lambda t: t.half().float()
    sd = {"image_proj.proj.weight": h(r(N * D, E) / E ** 0.5), "image_proj.proj.bias": h(r(N * D) * 0.3),
          "image_proj.norm.weight": h(1.0 + 0.1 * r(D)), "image_proj.norm.bias": h(0.1 * r(D))}
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    for p in R.block_prefixes(L):
        level = int(p.split(".")[1]) if p.startswith("down") else 3 if p.startswith("mid") else 3 - int(p.split(".")[1])
        C = boc[level]
        sd[p + PROC + "to_k_ip.weight"] = h(r(C, D) * k_scale / D ** 0.5)
        sd[p + PROC + "to_v_ip.weight"] = h(r(C, D) * v_scale / D ** 0.5)
    return sd


def to_diffusers(sd_ip, layers_per_block=2, numbered=True):
    """the adapter in diffusers' nested {"image_proj", "ip_adapter"} layout, with numbered ("<2k+1>.to_k_ip.weight", attn_processors order:
    down, up, mid) or module-named keys -- written independently of ladi_vton_amd.ip_adapter.numbered_order"""
    L = layers_per_block
    order = (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] +
             ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)] + ["mid_block.attentions.0"])
    proj = {k[len("image_proj."):]: v for k, v in sd_ip.items() if k.startswith("image_proj.")}
    ada = {}
    for k, v in sd_ip.items():
        if PROC in k:
            p, name = k.split(PROC)
            ada["%d.%s" % (2 * order.index(p) + 1, name) if numbered else k] = v
    return {"image_proj": proj, "ip_adapter": ada}


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, ip=None, pag_scale=0.0,
                    pag_adaptive_scale=0.0, layers=("mid",), guidance=7.5, table=None, freeu=None, callback=None, int_layers=(1, 2, 3, 4, 5),
                    counts=None):
    """pag_ref.tryon_reference with the image prompt: ip = (sd_ip, embeds [B, E], negative embeds [B, E] or None = zeros, scales) or None.
    Every sample group has its image tokens: the uncond group image_proj(negative), the cond and the perturbed group image_proj(embeds)."""
    if ip is None:
        return R.tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, pag_scale, pag_adaptive_scale,
                                 layers, guidance, table, 0.0, freeu, False, callback, int_layers, counts)
    sd_ip, emb, neg, scales = ip
    tok_c = image_proj(sd_ip, emb)
    tok_u = image_proj(sd_ip, torch.zeros_like(emb) if neg is None else neg)
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler)
    sch.set_timesteps(num_inference_steps)
    n = len(sch.timesteps)
    table = [float(guidance)] * n if table is None else list(table)
    assert len(table) == n
    ptab = R.pag_plan(pag_scale, pag_adaptive_scale, sch.timesteps)
    sel = R.layer_prefixes(layers, unet_cfg["layers_per_block"])
    do_cfg = any(G.is_cfg(g) for g in table)
    pe_c, pe_u = inp["prompt_embeds"], inp["negative_prompt_embeds"]
    mask_image[mask_image < 0.5] = 0
    mask_image[mask_image >= 0.5] = 1
    masked_image = image.float() * (mask_image < 0.5)
    pose = F.interpolate(pose_map, size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
    mom, _ = M.vae_encode(vae_sd, vae_cfg, cloth)
    cloth_latents = sf * M.posterior_sample(mom, inp["noise_cloth"])
    latents = inp["noise_latents"] * sch.init_noise_sigma
    mask_lat = F.interpolate(mask_image, size=(h, w))
    mom, feats = M.vae_encode(vae_sd, vae_cfg, masked_image)
    masked_lat = sf * M.posterior_sample(mom, inp["noise_masked"])
    inter = None
    if emasc_sd is not None:
        inter = M.mask_features(M.emasc_forward(emasc_sd, [feats[i] for i in int_layers]), mask_image)
    static_c = torch.cat([mask_lat, masked_lat, pose, cloth_latents], dim=1)
    static_u = torch.cat([mask_lat, masked_lat, torch.zeros_like(pose), torch.zeros_like(cloth_latents)], dim=1)
    n_cond = n_pag = 0
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        pag_i = ptab[i] > 0.0
        xs = sch.scale_model_input(latents, t)
        groups = ([torch.cat([xs, static_u], dim=1)] if cfg_i else []) + [torch.cat([xs, static_c], dim=1)] * (2 if pag_i else 1)
        ctx = ([pe_u] if cfg_i else []) + [pe_c] * (2 if pag_i else 1)
        tok = ([tok_u] if cfg_i else []) + [tok_c] * (2 if pag_i else 1)
        first = (len(groups) - 1) * B if pag_i else None
        eps = unet_forward(unet_sd, unet_cfg, torch.cat(groups), t, torch.cat(ctx), sel, first, freeu, (sd_ip, torch.cat(tok), scales))
        parts = list(eps.chunk(len(groups)))
        ep = parts.pop() if pag_i else None
        ec = parts.pop()
        eu = parts.pop() if cfg_i else None
        latents = sch.step(R.guided_eps(eu, ec, ep, table[i], ptab[i], 0.0), t, latents).prev_sample
        if callback is not None:
            latents = callback(i, latents)
        n_cond += 0 if cfg_i else 1
        n_pag += 1 if pag_i else 0
    if counts is not None:
        counts.update(cond_only=n_cond, pag=n_pag, evals=n, pag_table=ptab)
    img = M.vae_decode(vae_sd, vae_cfg, latents / sf, list(inter) if inter is not None else None,
                       list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents


def tryon_reference_cached(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, interval, branch, num_inference_steps, scheduler, ip, guidance=7.5,
                           table=None, counts=None):
    """tests/feature_cache_ref.py tryon_reference (the deep-feature cache's loop) with the image prompt.  That loop reaches every transformer
    block through oracle.models.transformer2d: for the span of the call the name is bound to this module's transformer2d with the tokens of
    the rows the evaluation runs over (B rows: the cond group; 2B: [uncond ; cond]), and put back afterwards."""
    from tests import feature_cache_ref as FC
    sd_ip, emb, neg, scales = ip
    B = emb.shape[0]
    tok_c = image_proj(sd_ip, emb)
    tok_all = torch.cat([image_proj(sd_ip, torch.zeros_like(emb) if neg is None else neg), tok_c])
    index = {b: i for i, b in enumerate(R.block_prefixes(unet_cfg["layers_per_block"]))}
    orig = M.transformer2d

    def with_image_term(sd, p, x, ehs, heads, groups):
        s = float(scales[index[p]])
        return transformer2d(sd, p, x, ehs, heads, groups, None, (sd_ip, tok_c if x.shape[0] == B else tok_all, s) if s != 0.0 else None)
    M.transformer2d = with_image_term
    try:
        return FC.tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, interval, branch, num_inference_steps, scheduler,
                                  guidance=guidance, table=table, counts=counts)
    finally:
        M.transformer2d = orig
