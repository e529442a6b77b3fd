"""Reference for FreeU (diffusers UNet2DConditionModel.enable_freeu): the yardstick tests/test_cpu_freeu.py and tests/test_gpu_freeu.py
compare the library with.  fourier_filter is diffusers' torch.fft formulation in float64, fourier_filter_direct the closed form the kernel
computes; the UNet forward is tests/feature_cache_ref.py's composition of oracle.models' block functions (any latent size, capture / shallow
modes) with apply_freeu before every concatenation of up_blocks.0 and up_blocks.1; the loop is feature_cache_ref.tryon_reference's with
this forward.  Nothing here imports the package under test except its scheduler mirrors (as tests/strength_ref.py does).

    freeu                    None (off) or (s1, s2, b1, b2), diffusers' argument order: stage i uses s = freeu[i], b = freeu[2 + i]
    apply_freeu(i, h, sk)    i >= 2 or freeu None: unchanged; else h[:, :C // 2] * b and fourier_filter(sk, threshold = 1, scale = s)
"""
import math

import torch
import torch.nn.functional as F

from oracle import models as M
from tests import feature_cache_ref as FR
from tests import guidance_ref as G
from tests import strength_ref as SR


def fourier_filter(x, threshold, scale):
    """diffusers.utils.torch_utils.fourier_filter on [B, C, H, W], in float64 -> float64"""
    x = x.double()
    B, C, H, W = x.shape
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = torch.fft.ifftshift(xf * mask, dim=(-2, -1))
    return torch.fft.ifftn(xf, dim=(-2, -1)).real


def low_pass(x):
    """the part of x [.., H, W] at the frequencies of fourier_filter's box for threshold 1: u in {0, -1 mod H}, v in {0, -1 mod W}, each
    distinct frequency once (an axis of length 1 has one, an axis of length 2 its mean and its Nyquist frequency); float64, no FFT"""
    x = x.double()
    H, W = x.shape[-2:]
    ys, xs = torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64)
    lp = torch.zeros_like(x)
    for u in sorted({0, (-1) % H}):
        for v in sorted({0, (-1) % W}):
            ey = torch.exp(-2j * math.pi * u * ys / H)
            ex = torch.exp(-2j * math.pi * v * xs / W)
            f = torch.einsum("...yx,y,x->...", x.to(torch.complex128), ey, ex)
            lp = lp + (f[..., None, None] * ey.conj()[:, None] * ex.conj()[None, :]).real
    return lp / (H * W)


def fourier_filter_direct(x, scale):
    """fourier_filter(x, 1, scale) in closed form: x + (scale - 1) low_pass(x)"""
    return x.double() + (scale - 1.0) * low_pass(x)


def apply_freeu(i, hidden, skip, freeu):
    """diffusers.utils.torch_utils.apply_freeu for up block i -> (hidden, skip), in the dtype they came in"""
    if freeu is None or i >= 2:
        return hidden, skip
    s, b = float(freeu[i]), float(freeu[2 + i])
    half = hidden.shape[1] // 2
    hidden = torch.cat([(hidden[:, :half].double() * b).to(hidden.dtype), hidden[:, half:]], dim=1)
    return hidden, fourier_filter(skip, 1, s).to(skip.dtype)


def unet_forward(sd, cfg, sample, timestep, ehs, freeu=None, mode=None, branch=0, cache=None):
    """feature_cache_ref.unet_forward (mode None / "capture" / "shallow") with apply_freeu before each concatenation of up_blocks.0 and
    up_blocks.1.  A shallow forward runs neither stage, so FreeU does not touch it."""
    assert mode in (None, "capture", "shallow")
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G_, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    k = int(branch)
    assert 0 <= k <= L
    shallow = mode == "shallow"
    n = sample.shape[0]
    forward_upsample_size = any(s % 8 != 0 for s in sample.shape[-2:])
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = M.conv(sd, "conv_in", sample)
    skips = [x]
    for i in range(4):
        for j in range(L):
            if shallow and (i > 0 or j >= k):
                continue
            x = M.resnet(sd, "down_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i < 3:
                x = M.transformer2d(sd, "down_blocks.%d.attentions.%d" % (i, j), x, ehs, heads[i], G_)
            skips.append(x)
        if i < 3 and not shallow:
            x = M.conv(sd, "down_blocks.%d.downsamplers.0.conv" % i, x, stride=2, padding=1)
            skips.append(x)
    if not shallow:
        x = M.resnet(sd, "mid_block.resnets.0", x, temb, G_, eps)
        x = M.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads[3], G_)
        x = M.resnet(sd, "mid_block.resnets.1", x, temb, G_, eps)
    captured = None
    for i in range(4):
        for j in range(L + 1):
            cache_pt = i == 3 and j == L - k
            if shallow and not cache_pt and (i < 3 or j < L - k):
                continue
            if cache_pt:
                if shallow:
                    assert cache.shape == (n, boc[1 if k == L else 0]) + tuple(sample.shape[-2:]), (cache.shape, sample.shape)
                    x = cache
                else:
                    captured = x.clone()
            x, sk = apply_freeu(i, x, skips.pop(), freeu)
            x = torch.cat([x, sk], dim=1)
            x = M.resnet(sd, "up_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i > 0:
                x = M.transformer2d(sd, "up_blocks.%d.attentions.%d" % (i, j), x, ehs, heads[3 - i], G_)
        if i < 3 and not shallow:
            if forward_upsample_size:
                x = F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = M.conv(sd, "up_blocks.%d.upsamplers.0.conv" % i, x)
    assert not skips
    x = M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G_, eps)))
    return (x, captured) if mode == "capture" else x


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, freeu, num_inference_steps, scheduler, interval=None, branch=0,
                    guidance=7.5, int_layers=(1, 2, 3, 4, 5), counts=None):
    """feature_cache_ref.tryon_reference's loop (cloth_cond_rate 1, a scalar guidance, the whole schedule) with the forward above.
    interval None: the plain loop, every evaluation whole; an int or flags: the feature-cache plan, a whole evaluation applies FreeU and
    refreshes the cache, a shallow one reads it.  counts (a dict) receives shallow / evals."""
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler)
    sch.set_timesteps(num_inference_steps)
    n = len(sch.timesteps)
    do_cfg = G.is_cfg(float(guidance))
    flags = FR.plan(n, interval) if interval is not None else None
    pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]]) if do_cfg else inp["prompt_embeds"]
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
    if do_cfg:
        mask_lat, masked_lat = torch.cat([mask_lat] * 2), torch.cat([masked_lat] * 2)
        pose = torch.cat([torch.zeros_like(pose), pose])
        cloth_latents = torch.cat([torch.zeros_like(cloth_latents), cloth_latents])
    cache, n_shallow = None, 0
    for i, t in enumerate(sch.timesteps):
        x = torch.cat([latents] * 2) if do_cfg else latents
        x = sch.scale_model_input(x, t)
        x = torch.cat([x, mask_lat, masked_lat, pose, cloth_latents], dim=1)
        if flags is None:
            eps = unet_forward(unet_sd, unet_cfg, x, t, pe, freeu)
        elif flags[i]:
            eps, cache = unet_forward(unet_sd, unet_cfg, x, t, pe, freeu, "capture", branch)
        else:
            eps = unet_forward(unet_sd, unet_cfg, x, t, pe, freeu, "shallow", branch, cache)
            n_shallow += 1
        if do_cfg:
            eu, et = eps.chunk(2)
            eps = G.guided_eps(eu, et, float(guidance))
        latents = sch.step(eps, t, latents).prev_sample
    if counts is not None:
        counts.update(shallow=n_shallow, evals=n, flags=flags)
    img = M.vae_decode(vae_sd, vae_cfg, latents / sf, list(inter) if inter is not None else None,
                       list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
