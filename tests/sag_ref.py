"""Reference for self-attention guidance (diffusers StableDiffusionSAGPipeline, Hong et al. 2023), in float32 / float64 torch: the yardstick
tests/test_cpu_sag.py and tests/test_gpu_sag.py compare the library with.  Nothing here imports the package under test.

With a = alphas_cumprod[t] of an evaluation, x the latents the scheduler holds, b the base prediction (the unconditional one in a CFG
evaluation, else the conditional one) and, for the base group's samples, the SAG map of mid_block.attentions.0's self-attention

    P_h = softmax(Q_h K_h^T / sqrt(d)) over keys      s[j] = sum_i mean_h P_h[i, j]      m[j] = s[j] > 1

    x0  = (x - sqrt(1 - a) b) / sqrt(a)
    M   = nearest-upsample(m as [hm, wm]) to [h, w]                 (F.interpolate's default mode)
    x0d = blur9(x0) M + x0 (1 - M)                                  (depthwise 9 x 9 Gaussian, sigma 1, reflect padding 4)
    xd  = sqrt(a) x0d + sqrt(1 - a) b
    d   = UNet(xd with the base group's other channels, context rows and image tokens)
    e   = [u + g (c - u) | c] + sag_scale (b - d),   guidance rescale (CFG evaluations only) acting on the whole sum

The tiny checkpoint of the tests is random: its mid block attends close to uniformly and many s[j] sit near 1, where rounding decides the
threshold.  peaked() scales the mid block's attn1.to_q / to_k weights by QK_FACTOR, which makes the map peaked (s between ~0.03 and ~4);
every SAG test runs the library and this reference on that checkpoint, and tests/test_cpu_sag.py asserts the conditioning.
"""
import math

import torch
import torch.nn.functional as F

from oracle import models as M
from tests import guidance_ref as G
from tests import preserve_ref as PR
from tests import ref_unet as RU
from tests import strength_ref as SR

MID = "mid_block.attentions.0"
QK_FACTOR = 4.0


def peaked(sd, factor=QK_FACTOR):
    """a copy of a UNet state dict whose mid-block attn1.to_q / to_k weights are multiplied by `factor` (fp16-representable again)"""
    out = dict(sd)
    for k in ("to_q", "to_k"):
        key = MID + ".transformer_blocks.0.attn1.%s.weight" % k
        out[key] = (sd[key].float() * factor).half().float()
    return out


def map_size(h, w):
    """the mid block's map size: three stride-2 convolutions with padding 1"""
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def qk_of(sd, cfg, mid_in):
    """Q, K [n, T, C] of the mid block's attn1 from the input of mid_block.attentions.0 (the output of mid_block.resnets.0), in its dtype"""
    n, C, h, w = mid_in.shape
    t = M.group_norm(sd, MID + ".norm", mid_in, cfg["norm_num_groups"], 1e-6).permute(0, 2, 3, 1).reshape(n, h * w, C)
    t = M.linear(sd, MID + ".proj_in", t)
    b = MID + ".transformer_blocks.0"
    a = M.layer_norm(sd, b + ".norm1", t)
    return M.linear(sd, b + ".attn1.to_q", a), M.linear(sd, b + ".attn1.to_k", a)


def col_sums(q, k, heads):
    """s [n, T] of Q, K [n, T, heads * d], in their dtype"""
    n, T, C = q.shape
    d = C // heads
    qh = q.reshape(n, T, heads, d).transpose(1, 2)
    kh = k.reshape(n, T, heads, d).transpose(1, 2)
    p = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(d), dim=-1)
    return p.mean(dim=1).sum(dim=1)


def sag_sums(sd, cfg, mid_in):
    """s [n, T] from the input of mid_block.attentions.0; sd's and mid_in's dtype decide the arithmetic"""
    q, k = qk_of(sd, cfg, mid_in)
    return col_sums(q, k, cfg["num_heads"][3])


def mask_of(s):
    return (s > 1.0).to(torch.uint8)


def forward_with_map(sd, cfg, x, t, ehs, **kw):
    """ref_unet.unet_forward -> (eps, s [n, T]) with the map taken from the forward's own mid-block input"""
    seen = {}

    def observe(name, v):
        if name == "mid_block.resnets.0":
            seen["mid"] = v
        if kw.get("observe"):
            kw["observe"](name, v)
    eps = RU.unet_forward(sd, cfg, x, t, ehs, **dict(kw, observe=observe))
    return eps, sag_sums(sd, cfg, seen["mid"])


def forward_with_map_fp16(sd, cfg, x, t, ehs):
    """forward_with_map with checkpoint and activations in fp16 on the CPU (the sinusoidal timestep embedding, computed in float32 as in
    diffusers, is cast to fp16 as the library's first linear sees it) -> (eps, s) in float32"""
    sd16 = {k: v.half() for k, v in sd.items()}
    emb = M.timestep_embedding
    M.timestep_embedding = lambda tt, dim: emb(tt, dim).half()
    try:
        eps, s = forward_with_map(sd16, cfg, x.half(), t, ehs.half())
    finally:
        M.timestep_embedding = emb
    return eps.float(), s.float()


def band_of(sd, cfg, x, t, ehs):
    """-> (s float32 reference, band): the band around the threshold inside which the library's mask is not pinned -- twice the largest
    difference between the reference in float32 and the reference in fp16.  Reference against reference, never the code under test"""
    s32 = forward_with_map(sd, cfg, x, t, ehs)[1]
    s16 = forward_with_map_fp16(sd, cfg, x, t, ehs)[1]
    return s32, 2.0 * float((s32 - s16).abs().max())


def taps(dtype=torch.float64):
    """exp(-k^2 / 2), k = -4 .. 4, normalised to sum 1"""
    k = torch.arange(-4, 5, dtype=torch.float64)
    e = torch.exp(-0.5 * k * k)
    return (e / e.sum()).to(dtype)


def blur9(x):
    """depthwise 9 x 9 Gaussian, sigma 1, reflect padding 4, as two 1-D passes (rows of the padded image, then columns), in x's dtype"""
    n, C, h, w = x.shape
    assert h >= 5 and w >= 5, (h, w)
    t = taps(x.dtype)
    xp = F.pad(x, (4, 4, 4, 4), mode="reflect")
    xp = F.conv2d(xp, t.reshape(1, 1, 1, 9).expand(C, 1, 1, 9), groups=C)
    return F.conv2d(xp, t.reshape(1, 1, 9, 1).expand(C, 1, 9, 1), groups=C)


def upsampled(m, h, w):
    """m [B, hm, wm] -> [B, 1, h, w] in {0, 1}, F.interpolate's default (nearest) mode"""
    return F.interpolate(m.float().unsqueeze(1), size=(h, w))


def degrade(x, b, m, a):
    """steps 2-3: x, b [B, 4, h, w], m [B, hm, wm] (0 / 1), a a python float -> xd in x's dtype"""
    sa, s1 = math.sqrt(a), math.sqrt(1.0 - a)
    x0 = (x - s1 * b) / sa
    Mk = upsampled(m, x.shape[2], x.shape[3]).to(x.dtype)
    x0d = blur9(x0) * Mk + x0 * (1 - Mk)
    return sa * x0d + s1 * b


def combine(eu, ec, ed, g, s, phi=0.0):
    """step 5 in the inputs' dtype.  eu None: no CFG or a cond-only evaluation (the base is ec); ed None or s == 0: no SAG term.  The rescale
    (CFG evaluations only) takes its statistics of the whole sum, in float64, with the cond prediction"""
    e = ec if eu is None else eu + g * (ec - eu)
    if ed is not None and s != 0.0:
        e = e + s * ((ec if eu is None else eu) - ed)
    if eu is not None and phi > 0.0:
        e = (e.double() * G.rescale_factor(e, ec, phi)).to(e.dtype)
    return e


def sched_reference(sch, eps_seq, cfg, gtab, s, phi, lat0):
    """guidance_ref.sched_reference with the SAG combine.  eps_seq [evals, 3B or 2B, 4, h, w]: [uncond ; cond ; degraded] with cfg, else
    [cond ; degraded]; rows an evaluation must not read may hold NaN"""
    B = lat0.shape[0]
    x = lat0.double()
    for i, t in enumerate(sch.timesteps):
        o = B if cfg else 0
        ec = eps_seq[i, o:o + B].double()
        eu = eps_seq[i, :B].double() if cfg and G.is_cfg(gtab[i]) else None
        ed = eps_seq[i, o + B:o + 2 * B].double() if s != 0.0 else None
        x = sch.step(combine(eu, ec, ed, gtab[i] if cfg else 1.0, s, phi), t, x).prev_sample
    return x


def tryon_sag_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, *, sag_scale=0.0, guidance=7.5,
                        table=None, phi=0.0, freeu=None, ip=None, tome=None, init_latents=None, first_step=0, init_is_noisy=False,
                        preserve=None, cloth_cond_rate=1.0, no_pose=False, generator=None, int_layers=(1, 2, 3, 4, 5), callback=None,
                        forced_masks=None, info=None):
    """the plain loop of ref_tryon.tryon_reference (scheduler mirror, guidance table, rescale, strength, preserve, callback; FreeU, an image
    prompt and token merging as there) with steps 1-5 in every evaluation.  sag_scale = 0 runs no second forward and is tryon_reference bit
    for bit.  forced_masks: per evaluation, the m [B, hm, wm] to use in place of the reference's own.  info receives masks and sums (per
    evaluation, the base group's), noise_pred, latents, cond_only and evals"""
    from tests import ip_adapter_ref as IP
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    hm, wm = map_size(h, w)
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler) if isinstance(scheduler, str) else scheduler
    sch.set_timesteps(num_inference_steps, first_step=first_step) if first_step else sch.set_timesteps(num_inference_steps)
    n = len(sch.timesteps)
    table = [float(guidance)] * n if table is None else list(table)
    assert len(table) == n, (len(table), n)
    do_cfg = any(G.is_cfg(g) for g in table)
    bits, feather_sigma = (PR.MODES[preserve[0]], preserve[1]) if preserve is not None else (0, 0.0)
    pe_c, pe_u = inp["prompt_embeds"], inp["negative_prompt_embeds"]
    if ip is not None:
        sd_ip, emb, neg, scales = ip
        tok_c = IP.image_proj(sd_ip, emb)
        tok_u = IP.image_proj(sd_ip, torch.zeros_like(emb) if neg is None else neg)
    mask_image[mask_image < 0.5] = 0
    mask_image[mask_image >= 0.5] = 1
    mask = mask_image
    masked_image = image.float() * (mask < 0.5)
    pose = F.interpolate(pose_map, size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
    if no_pose:
        pose = torch.zeros_like(pose)
    cloth_latents = None
    if cloth is not None:
        mom, _ = M.vae_encode(vae_sd, vae_cfg, cloth)
        cloth_latents = sf * M.posterior_sample(mom, inp["noise_cloth"])
    if bits & 1:
        mom, _ = M.vae_encode(vae_sd, vae_cfg, image.float())
        z0 = sf * torch.chunk(mom, 2, dim=1)[0]
        keep, kc = PR.keep_mask(mask), PR.keep_coeffs(sch)
    if first_step > 0:
        k_x, k_n = (1.0, 0.0) if init_is_noisy else SR.start_coeffs(scheduler, sch)
        latents = SR.start_latents(init_latents, inp["noise_latents"], k_x, k_n, h, w).float()
    else:
        latents = inp["noise_latents"] * sch.init_noise_sigma
    tail = num_inference_steps - first_step
    cloth_off_from = tail - (1 - cloth_cond_rate) * tail if cloth_cond_rate is not None else float("inf")
    mask_lat = F.interpolate(mask, size=(h, w))
    mom, feats = M.vae_encode(vae_sd, vae_cfg, masked_image)
    masked_lat = sf * M.posterior_sample(mom, inp["noise_masked"])
    inter = None
    if emasc_sd is not None:
        inter = [feats[i] for i in int_layers]
        inter = M.emasc_forward(emasc_sd, inter)
        inter = M.mask_features(inter, mask_image)
    extra = {} if generator is None else {"generator": generator}
    n_cond = 0
    noise_pred, lat_seq, masks, sums = [], [], [], []
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        if cloth_latents is not None and i >= cloth_off_from:
            cloth_latents = torch.zeros_like(cloth_latents)
        xs = sch.scale_model_input(latents, t)
        opt = [cloth_latents] if cloth_latents is not None else []
        static_c = [mask_lat, masked_lat, pose] + opt
        static_u = [mask_lat, masked_lat, torch.zeros_like(pose)] + [torch.zeros_like(c) for c in opt]
        x_c, x_u = torch.cat([xs] + static_c, dim=1), torch.cat([xs] + static_u, dim=1)
        x = torch.cat(([x_u] if cfg_i else []) + [x_c])
        ehs = torch.cat(([pe_u] if cfg_i else []) + [pe_c])
        kw = dict(freeu=freeu)
        if ip is not None:
            kw["ip"] = (sd_ip, torch.cat(([tok_u] if cfg_i else []) + [tok_c]), scales)
        if tome is not None:
            kw["tome"] = (tome[0], tome[1][i] if tome[1] is not None else None, None, "proj_in")
        if sag_scale == 0.0:
            eps = RU.unet_forward(unet_sd, unet_cfg, x, t, ehs, **kw)
        else:
            eps, s_all = forward_with_map(unet_sd, unet_cfg, x, t, ehs, **kw)
        parts = list(eps.chunk(x.shape[0] // B))
        ec = parts.pop()
        eu = parts.pop() if cfg_i else None
        ed = None
        if sag_scale != 0.0:
            # the base group is the first B samples of this evaluation: uncond under CFG, else cond
            s_b = s_all[:B].reshape(B, hm, wm)
            m_b = mask_of(s_b) if forced_masks is None else forced_masks[i].to(torch.uint8)
            b = eu if cfg_i else ec
            a = float(sch.alphas_cumprod[int(round(float(t)))])
            xd = degrade(latents, b, m_b, a)
            kw2 = dict(freeu=freeu)
            if ip is not None:
                kw2["ip"] = (sd_ip, tok_u if cfg_i else tok_c, scales)
            if tome is not None:
                kw2["tome"] = (tome[0], None, None, "proj_in")
            x2 = torch.cat([sch.scale_model_input(xd, t)] + (static_u if cfg_i else static_c), dim=1)
            ed = RU.unet_forward(unet_sd, unet_cfg, x2, t, pe_u if cfg_i else pe_c, **kw2)
            masks.append(m_b)
            sums.append(s_b)
        eps = combine(eu, ec, ed, table[i], sag_scale, phi)
        out = sch.step(eps, t, latents, **extra)
        latents = out if torch.is_tensor(out) else out.prev_sample
        if bits & 1:
            latents = PR.blend(latents, keep, z0, inp["noise_latents"], *kc[i])
        if callback is not None:
            latents = callback(i, latents)
        n_cond += 0 if cfg_i else 1
        noise_pred.append(eps)
        lat_seq.append(latents)
    if info is not None:
        info.update(cond_only=n_cond, evals=n, noise_pred=noise_pred, latents=lat_seq, masks=masks, sums=sums)
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    if bits & 2:
        img = PR.composite(img, image, PR.feather(mask, feather_sigma) if feather_sigma > 0 else mask).float()
    else:
        img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
