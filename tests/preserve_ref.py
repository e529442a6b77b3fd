"""Reference for keeping the unmasked region (`preserve_unmasked`): the yardstick tests/test_cpu_preserve.py and tests/test_gpu_preserve.py
compare the library with.  float64 torch for the blend coefficients, the feathered mask and the composite; tryon_reference drives the oracle
modules with the package's scheduler mirrors, like tests/strength_ref.py and tests/feature_cache_ref.py.

    keep      = 1 - max_pool2d(binarised mask, 8)            a latent pixel whose whole 8x8 footprint is unmasked
    z0        = scaling_factor * mean(vae.encode(image))     the posterior mode of the full, unmasked image (no RNG draw)
    after the scheduler update of evaluation i (the latents then belong to timesteps[i + 1]):
        latents[keep] = k_x[i] z0 + k_n[i] noise             the scheduler's add_noise at timesteps[i + 1], noise = the initial-latents noise
        latents[keep] = z0                                   after the last evaluation
    the blend acts on scheduler.step(...).prev_sample only: scheduler state (PLMS cur_sample, the eps / data-prediction history) is not blended
    pixels:   out = M g + (1 - M) p, g = clamp(decoded / 2 + 0.5, 0, 1), p = clamp(image / 2 + 0.5, 0, 1), M the binarised mask or its separable
              Gaussian blur (radius ceil(3 sigma), weights normalised in float64, replicate border); M == 0 / 1 select p / g
"""
import math

import torch
import torch.nn.functional as F

from oracle import models as M
from tests import feature_cache_ref as FC
from tests import guidance_ref as G
from tests import strength_ref as SR

SCHEDULERS = SR.SCHEDULERS
MODES = {None: 0, "latents": 1, "pixels": 2, "both": 3}


def keep_coeffs(sch):
    """float64 [(k_x, k_n)] * evals for a mirror `sch` with set_timesteps done: add_noise's coefficients at timesteps[i + 1], read off the
    mirror's own add_noise (x0 = 1, noise = 0 and the reverse); the last row is (1, 0)"""
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    n = len(sch.timesteps)
    out = []
    for i in range(n):
        if i + 1 < n:
            t = sch.timesteps[i + 1]
            out.append((float(sch.add_noise(one, zero, t)), float(sch.add_noise(zero, one, t))))
        else:
            out.append((1.0, 0.0))
    return out


def binarise(mask):
    return (mask >= 0.5).to(torch.float32)


def keep_mask(mask):
    """bool [B, 1, H / 8, W / 8] from a mask [B, 1, H, W]"""
    return F.max_pool2d(binarise(mask), 8) < 0.5


def blend(latents, keep, z0, noise, k_x, k_n):
    """the select of the latent blend, in latents' dtype; (1, 0) stores z0 itself"""
    known = z0.double() if (k_x, k_n) == (1.0, 0.0) else k_x * z0.double() + k_n * noise.double()
    return torch.where(keep, known.to(latents.dtype), latents)


def sched_reference(sch, eps_seq, table, phi, lat0, keep, z0, noise, generator=None, seen=None):
    """tests/guidance_ref.py sched_reference with the blend after every step (float64).  keep bool [B, 1, h, w]; seen (a list) receives the
    blended latents of every evaluation"""
    B = lat0.shape[0]
    x = lat0.double()
    extra = {} if generator is None else {"generator": generator}
    assert len(table) == len(sch.timesteps) == eps_seq.shape[0]
    kc = keep_coeffs(sch)
    for i, t in enumerate(sch.timesteps):
        ec = eps_seq[i, B:].double()
        e = G.guided_eps(eps_seq[i, :B].double(), ec, table[i], phi) if G.is_cfg(table[i]) else ec
        x = sch.step(e, t, x, **extra).prev_sample
        x = blend(x, keep, z0, noise, *kc[i])
        if seen is not None:
            seen.append(x.clone())
    return x


def feather_weights(sigma):
    """float64 [2 r + 1], r = ceil(3 sigma), normalised"""
    r = int(math.ceil(3.0 * sigma))
    k = torch.arange(-r, r + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * k * k / (sigma * sigma))
    return w / w.sum(), r


def feather(mask_bin, sigma):
    """float64 separable Gaussian blur of a binarised mask [B, 1, H, W], replicate border"""
    w, r = feather_weights(sigma)
    m = F.conv2d(F.pad(mask_bin.double(), (r, r, 0, 0), mode="replicate"), w.view(1, 1, 1, -1))
    return F.conv2d(F.pad(m, (0, 0, r, r), mode="replicate"), w.view(1, 1, -1, 1))


def post(x):
    """clamp(x / 2 + 0.5, 0, 1) in float64"""
    return (x.double() / 2 + 0.5).clamp(0, 1)


def composite(decoded, image, m):
    """float64 [B, H, W, 3] from decoded / image [B, 3, H, W] (values in [-1, 1] before post) and m [B, 1, H, W]"""
    g, p, m = post(decoded), post(image), m.double()
    out = torch.where(m == 0, p, torch.where(m == 1, g, m * g + (1 - m) * p))
    return out.permute(0, 2, 3, 1)


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, mode, num_inference_steps, scheduler, feather_sigma=0.0, guidance=7.5,
                    table=None, init_latents=None, first_step=0, interval=None, branch=0, cloth_cond_rate=1.0, generator=None,
                    int_layers=(1, 2, 3, 4, 5), seen=None):
    """tests/feature_cache_ref.py tryon_reference (the oracle modules, the mirror scheduler over its evaluations, a guidance `table`, an
    optional start at first_step, an optional feature-cache plan) with the latent blend after every scheduler step and the composite after the
    decode.  mode: None, "latents", "pixels" or "both"; None is the reference it restates.  seen (a list) receives every evaluation's latents."""
    bits = MODES[mode]
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler)
    sch.set_timesteps(num_inference_steps, first_step=first_step) if first_step else sch.set_timesteps(num_inference_steps)
    n = len(sch.timesteps)
    table = [float(guidance)] * n if table is None else list(table)
    assert len(table) == n, (len(table), n)
    do_cfg = any(G.is_cfg(g) for g in table)
    co = [do_cfg and not G.is_cfg(g) for g in table]
    flags = FC.plan(n, interval, co) if interval is not None else None
    pe_c = inp["prompt_embeds"]
    pe = torch.cat([inp["negative_prompt_embeds"], pe_c]) if do_cfg else pe_c
    mask_image[mask_image < 0.5] = 0
    mask_image[mask_image >= 0.5] = 1
    mask = mask_image
    masked_image = image.float() * (mask < 0.5)
    pose = F.interpolate(pose_map, size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
    cloth_latents = None
    if cloth is not None:
        mom, _ = M.vae_encode(vae_sd, vae_cfg, cloth)
        cloth_latents = sf * M.posterior_sample(mom, inp["noise_cloth"])
    if bits & 1:
        mom, _ = M.vae_encode(vae_sd, vae_cfg, image.float())
        z0 = sf * torch.chunk(mom, 2, dim=1)[0]
        keep, kc = keep_mask(mask), keep_coeffs(sch)
    if first_step > 0:
        k_x, k_n = SR.start_coeffs(scheduler, sch)
        latents = SR.start_latents(init_latents, inp["noise_latents"], k_x, k_n, h, w).float()
    else:
        latents = inp["noise_latents"] * sch.init_noise_sigma
    tail = num_inference_steps - first_step
    cloth_conditioning_steps = (1 - cloth_cond_rate) * tail
    mask_lat = F.interpolate(mask, size=(h, w))
    mom, feats = M.vae_encode(vae_sd, vae_cfg, masked_image)
    masked_lat = sf * M.posterior_sample(mom, inp["noise_masked"])
    inter = None
    if emasc_sd is not None:
        inter = [feats[i] for i in int_layers]
        inter = M.emasc_forward(emasc_sd, inter)
        inter = M.mask_features(inter, mask_image)
    if do_cfg:
        mask_lat = torch.cat([mask_lat] * 2)
        masked_lat = torch.cat([masked_lat] * 2)
        pose = torch.cat([torch.zeros_like(pose), pose])
        if cloth_latents is not None:
            cloth_latents = torch.cat([torch.zeros_like(cloth_latents), cloth_latents])
    extra = {} if generator is None else {"generator": generator}
    cache = None
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        x = torch.cat([latents] * 2) if cfg_i else latents
        if cloth_latents is not None and i >= (tail - cloth_conditioning_steps):
            cloth_latents = torch.zeros_like(cloth_latents)
        x = sch.scale_model_input(x, t)
        parts = [mask_lat, masked_lat, pose] + ([cloth_latents] if cloth_latents is not None else [])
        sub = do_cfg and not cfg_i
        if sub:
            parts = [p[B:] for p in parts]
        x = torch.cat([x] + parts, dim=1)
        ehs = pe_c if sub else pe
        rows = slice(B, 2 * B) if sub else slice(0, 2 * B if do_cfg else B)
        if flags is None:
            eps = M.unet_forward(unet_sd, unet_cfg, x, t, ehs)
        elif flags[i]:
            eps, cap = FC.unet_forward(unet_sd, unet_cfg, x, t, ehs, "capture", branch)
            if cache is None:
                cache = torch.full(((2 * B if do_cfg else B),) + tuple(cap.shape[1:]), float("nan"))
            cache[rows] = cap
        else:
            eps = FC.unet_forward(unet_sd, unet_cfg, x, t, ehs, "shallow", branch, cache[rows])
        if cfg_i:
            eu, et = eps.chunk(2)
            eps = G.guided_eps(eu, et, table[i])
        latents = sch.step(eps, t, latents, **extra).prev_sample
        if bits & 1:
            latents = blend(latents, keep, z0, inp["noise_latents"], *kc[i])
        if seen is not None:
            seen.append(latents.clone())
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    if bits & 2:
        m = feather(mask, feather_sigma) if feather_sigma > 0 else mask
        img = composite(img, image, m).float()
    else:
        img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
