"""Reference for starting the try-on loop from an image or latents (`strength`): the yardstick tests/test_cpu_strength.py and
tests/test_gpu_strength.py compare the library with.  The step arithmetic, the resample and the start latents are restated here in
float64; tryon_reference drives the oracle modules with the package's scheduler mirrors (set_timesteps(n, first_step=)), whose tails
tests/test_cpu_strength.py pins against the native tables.

    init_timestep = min(int(N * strength), N)        diffusers' get_timesteps, Python float64
    first_step    = N - init_timestep                the run is the evaluations of steps first_step .. of the N-step schedule
    resample      F.interpolate(mode="bilinear", align_corners=False): source coordinate max((o + 0.5) * in / out - 0.5, 0), lower
                  neighbour floor(src), upper one clamped to the last row / column, no antialias; equal sizes: the tensor itself
    x_start       = k_x * resample(init) + k_n * noise
                  DDIM / PNDM / DPM-Solver++: k_x = sqrt(a_t), k_n = sqrt(1 - a_t) at t = timesteps[first_step]
                  LMS / Euler / Euler-ancestral: k_x = 1, k_n = sigma[first_step]
                  init_is_noisy: k_x = 1, k_n = 0 (the init is the loop's latents at that step)
"""
import math

import torch
import torch.nn.functional as F

from oracle import models as M
from oracle import pipeline as P
from tests import guidance_ref as G

SCHEDULERS = ("ddim", "pndm", "lms", "dpmpp2m", "euler", "euler_a")
SIGMA_KINDS = ("lms", "euler", "euler_a")


def first_step_of(strength, n):
    init_timestep = min(int(n * float(strength)), n)
    return n - init_timestep


def _axis(n_in, n_out):
    """-> (i0, i1, lam) of every output index along one axis, float64"""
    o = torch.arange(n_out, dtype=torch.float64)
    src = ((o + 0.5) * n_in / n_out - 0.5).clamp(min=0.0)
    i0 = src.floor().clamp(max=n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.double()


def resample(x, h, w):
    """x [B, C, hs, ws] -> float64 [B, C, h, w]"""
    x = x.double()
    hs, ws = x.shape[2:]
    if (hs, ws) == (h, w):
        return x
    y0, y1, ly = _axis(hs, h)
    x0, x1, lx = _axis(ws, w)
    ly, lx = ly.view(1, 1, h, 1), lx.view(1, 1, 1, w)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


def start_latents(init, noise, k_x, k_n, h, w):
    """float64 [B, 4, h, w]; noise may be None when k_n == 0"""
    x = k_x * resample(init, h, w)
    return x if k_n == 0 else x + k_n * noise.double()


def make_mirror(name):
    import ladi_vton_amd as L
    return {"ddim": L.DDIMScheduler, "pndm": L.PNDMScheduler, "lms": L.LMSDiscreteScheduler, "dpmpp2m": L.DPMSolverMultistepScheduler,
            "euler": L.EulerDiscreteScheduler, "euler_a": L.EulerAncestralDiscreteScheduler}[name]()


def start_coeffs(name, sch):
    """(k_x, k_n) in float64 for a mirror `sch` whose set_timesteps(n, first_step=) is done"""
    if name in SIGMA_KINDS:
        return 1.0, float(sch.sigmas[0])
    a = float(P.alphas_cumprod()[int(sch.timesteps[0])].double())
    return math.sqrt(a), math.sqrt(1.0 - a)


def synthetic_init(B, hs, ws, seed=77):
    """smooth latents of the magnitude the tiny model's loop holds: a low-resolution field, upsampled, plus a little white noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((B, 4, max(hs // 4, 1), max(ws // 4, 1)), generator=g)
    x = F.interpolate(low, size=(hs, ws), mode="bilinear", align_corners=False)
    return (x + 0.1 * torch.randn((B, 4, hs, ws), generator=g)).float()


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, init_latents, first_step, num_inference_steps, scheduler,
                    guidance=7.5, table=None, init_is_noisy=False, cloth_cond_rate=1.0, generator=None, int_layers=(1, 2, 3, 4, 5),
                    seen=None):
    """tests/guidance_ref.py tryon_reference started at step first_step of the schedule from start_latents(init_latents, ..): the oracle
    modules, the mirror scheduler `scheduler` (a name of SCHEDULERS) over its tail.  table: one guidance scale per tail evaluation (None:
    `guidance` for all).  generator: for the mirrors whose step() draws noise.  seen (a list) receives (i, t) of every evaluation.
    first_step = 0 ignores the init: the plain run."""
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = make_mirror(scheduler)
    sch.set_timesteps(num_inference_steps, first_step=first_step)
    n = len(sch.timesteps)
    table = [float(guidance)] * n if table is None else list(table)
    assert len(table) == n, (len(table), n)
    do_cfg = any(G.is_cfg(g) for g in table)
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
    if first_step > 0:
        k_x, k_n = (1.0, 0.0) if init_is_noisy else start_coeffs(scheduler, sch)
        latents = start_latents(init_latents, inp["noise_latents"], k_x, k_n, h, w).float()
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
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        x = torch.cat([latents] * 2) if cfg_i else latents
        if cloth_latents is not None and i >= (tail - cloth_conditioning_steps):
            cloth_latents = torch.zeros_like(cloth_latents)
        x = sch.scale_model_input(x, t)
        parts = [mask_lat, masked_lat, pose] + ([cloth_latents] if cloth_latents is not None else [])
        if do_cfg and not cfg_i:
            parts = [p[B:] for p in parts]
        x = torch.cat([x] + parts, dim=1)
        eps = M.unet_forward(unet_sd, unet_cfg, x, t, pe if cfg_i or not do_cfg else pe_c)
        if cfg_i:
            eu, et = eps.chunk(2)
            eps = G.guided_eps(eu, et, table[i])
        latents = sch.step(eps, t, latents, **extra).prev_sample
        if seen is not None:
            seen.append((i, float(t)))
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
