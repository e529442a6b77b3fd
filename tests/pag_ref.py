"""Reference for perturbed-attention guidance (diffusers PAGMixin with PAGIdentitySelfAttnProcessor2_0 / PAGCFGIdentitySelfAttnProcessor2_0):
the yardstick tests/test_cpu_pag.py and tests/test_gpu_pag.py compare the library with.  The UNet forward is tests/freeu_ref.py's
composition of oracle.models' block functions (any latent size, optional FreeU) with a transformer2d whose self-attention is the identity
map (O = V) for the samples >= pag_first in the selected blocks; the loop is the guidance / preserve references' loop with a third sample
group.  Nothing here imports the package under test except its scheduler mirrors (as tests/strength_ref.py does).

    layers      the selected blocks as a set of diffusers module prefixes ("mid_block.attentions.0", "down_blocks.1.attentions.0", ..),
                from layer_prefixes(names, layers_per_block) with the names `pag_applied_layers` takes
    pag_first   samples [pag_first, n) of a forward are perturbed; None or >= n: none
    e = u + g (c - u) + s (c - p)      CFG evaluation           e = c + s (c - p)      no CFG, or a cond-only evaluation of a guided run
    rescale acts on the three-term sum of CFG evaluations (guidance_ref.rescale_factor with the cond prediction)
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from tests import freeu_ref as FU
from tests import guidance_ref as G
from tests import preserve_ref as PR
from tests import strength_ref as SR


def block_prefixes(layers_per_block=2):
    """the transformer blocks in execution order: bit i of the library's mask is entry i"""
    L = layers_per_block
    return (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] + ["mid_block.attentions.0"] +
            ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)])


def layer_prefixes(names, layers_per_block=2):
    """`pag_applied_layers` names -> the set of module prefixes they select, written independently of pipeline.pag_layer_mask: a name
    "down.block_1.attentions_0" selects the prefixes that start with "down_blocks.1.attentions.0", "mid" the mid block"""
    if isinstance(names, str):
        names = [names]
    out = set()
    every = block_prefixes(layers_per_block)
    for name in names:
        p = name.split(".")
        if name == "mid":
            sel = {"mid_block.attentions.0"}
        elif len(p) == 1:
            sel = {b for b in every if b.startswith(p[0] + "_blocks.")}
        elif len(p) == 2:
            sel = {b for b in every if b.startswith(p[0] + "_blocks." + p[1][len("block_"):] + ".attentions.")}
        else:
            sel = {b for b in every if b == p[0] + "_blocks." + p[1][len("block_"):] + ".attentions." + p[2][len("attentions_"):]}
        assert sel, name
        out |= sel
    return out


def mask_of(prefixes, layers_per_block=2):
    return sum(1 << i for i, b in enumerate(block_prefixes(layers_per_block)) if b in prefixes)


def transformer2d(sd, p, x, ehs, heads, groups, perturbed_from=None):
    """oracle.models.transformer2d with attention(q, k, v) swapped for v in attn1 on the samples [perturbed_from, n)"""
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
    t = M.linear(sd, b + ".attn2.to_out.0", M.attention(M.linear(sd, b + ".attn2.to_q", a), M.linear(sd, b + ".attn2.to_k", ehs),
                                                        M.linear(sd, b + ".attn2.to_v", ehs), heads)) + t
    a = M.layer_norm(sd, b + ".norm3", t)
    u, g = M.linear(sd, b + ".ff.net.0.proj", a).chunk(2, dim=-1)
    t = M.linear(sd, b + ".ff.net.2", u * F.gelu(g)) + t
    t = M.linear(sd, p + ".proj_out", t)
    return t.reshape(n, h, w, C).permute(0, 3, 1, 2) + res


def unet_forward(sd, cfg, sample, timestep, ehs, layers=(), pag_first=None, freeu=None):
    """freeu_ref.unet_forward's whole forward (any latent size) with the perturbed transformer in the blocks `layers`"""
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G_, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    n = sample.shape[0]
    layers = set(layers)

    def xf(p, x, hd):
        return transformer2d(sd, p, x, ehs, hd, G_, pag_first if p in layers else None)
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


def pag_plan(pag_scale, pag_adaptive_scale, timesteps):
    """PAGMixin._get_pag_scale per evaluation"""
    if pag_adaptive_scale == 0:
        return [float(pag_scale)] * len(timesteps)
    return [max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(t)), 0.0) for t in timesteps]


def guided_eps(eu, ec, ep, g, s, phi=0.0):
    """the combine of one evaluation in the inputs' dtype.  eu None: no CFG or a cond-only evaluation; ep None (s == 0): no PAG.  The
    rescale (CFG evaluations only) takes its statistics of the three-term sum, in float64"""
    e = ec if eu is None else eu + g * (ec - eu)
    if ep is not None and s > 0.0:
        e = e + s * (ec - ep)
    if eu is not None and phi > 0.0:
        e = (e.double() * G.rescale_factor(e, ec, phi)).to(e.dtype)
    return e


def sched_reference(sch, eps_seq, cfg, gtab, ptab, phi, lat0):
    """guidance_ref.sched_reference with the PAG combine.  eps_seq [evals, 3B or 2B, 4, h, w]: [uncond ; cond ; perturbed] with cfg, else
    [cond ; perturbed]; rows an evaluation must not read may hold NaN"""
    B = lat0.shape[0]
    x = lat0.double()
    for i, t in enumerate(sch.timesteps):
        o = B if cfg else 0
        ec = eps_seq[i, o:o + B].double()
        eu = eps_seq[i, :B].double() if cfg and G.is_cfg(gtab[i]) else None
        ep = eps_seq[i, o + B:o + 2 * B].double() if ptab[i] > 0.0 else None
        x = sch.step(guided_eps(eu, ec, ep, gtab[i] if cfg else 1.0, ptab[i], phi), t, x).prev_sample
    return x


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, pag_scale=0.0, pag_adaptive_scale=0.0,
                    layers=("mid",), guidance=7.5, table=None, phi=0.0, freeu=None, preserve_latents=False, callback=None,
                    int_layers=(1, 2, 3, 4, 5), counts=None):
    """the try-on loop (oracle modules, the mirror scheduler, cloth_cond_rate 1) with 3B or 2B sample groups: an evaluation with s_i > 0
    runs [uncond ; cond ; perturbed] (or [cond ; perturbed] without CFG or cond-only), one with s_i == 0 runs without the perturbed group.
    table: a guidance scale per evaluation (None: `guidance`); preserve_latents: the latent blend of preserve_ref; callback(i, latents) ->
    latents after every evaluation.  counts (a dict) receives cond_only / pag evaluation counts."""
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
    ptab = pag_plan(pag_scale, pag_adaptive_scale, sch.timesteps)
    sel = layer_prefixes(layers, unet_cfg["layers_per_block"])
    do_cfg = any(G.is_cfg(g) for g in table)
    pe_c, pe_u = inp["prompt_embeds"], inp["negative_prompt_embeds"]
    mask_image[mask_image < 0.5] = 0
    mask_image[mask_image >= 0.5] = 1
    masked_image = image.float() * (mask_image < 0.5)
    pose = F.interpolate(pose_map, size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
    mom, _ = M.vae_encode(vae_sd, vae_cfg, cloth)
    cloth_latents = sf * M.posterior_sample(mom, inp["noise_cloth"])
    if preserve_latents:
        mom, _ = M.vae_encode(vae_sd, vae_cfg, image.float())
        z0 = sf * torch.chunk(mom, 2, dim=1)[0]
        keep, kc = PR.keep_mask(mask_image), PR.keep_coeffs(sch)
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
        first = (len(groups) - 1) * B if pag_i else None
        eps = unet_forward(unet_sd, unet_cfg, torch.cat(groups), t, torch.cat(ctx), sel, first, freeu)
        parts = list(eps.chunk(len(groups)))
        ep = parts.pop() if pag_i else None
        ec = parts.pop()
        eu = parts.pop() if cfg_i else None
        latents = sch.step(guided_eps(eu, ec, ep, table[i], ptab[i], phi), t, latents).prev_sample
        if preserve_latents:
            latents = PR.blend(latents, keep, z0, inp["noise_latents"], *kc[i])
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
