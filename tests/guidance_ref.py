"""Reference for the guidance schedule, the CFG cut-off and guidance rescale: the yardstick tests/test_cpu_guidance.py and
tests/test_gpu_guidance.py compare the library with.  float64 torch for the statistics; nothing here imports the package under test.

    e_i = u + g_i (c - u)                                   for a CFG evaluation (g_i > 1)
    e_i = e_i * (phi * std(c) / std(e_i) + (1 - phi))       guidance rescale, per sample over all its elements, torch.std's default
                                                            (unbiased) correction, no epsilon
    e_i = c                                                 for a cond-only evaluation (g_i <= 1): the unconditional half is not evaluated,
                                                            the rule tryon_pipe.py applies to a whole run (do_classifier_free_guidance)
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from oracle import pipeline as P


def is_cfg(g):
    return g > 1.0


def rescale_factor(e, ec, phi):
    """[n, 1, ...] float64: phi * std(ec) / std(e) + (1 - phi) per sample"""
    dims = list(range(1, e.ndim))
    return phi * (ec.double().std(dim=dims, keepdim=True) / e.double().std(dim=dims, keepdim=True)) + (1.0 - phi)


def guided_eps(eu, ec, g, phi=0.0):
    """eu, ec: [n, ...] unconditional / conditional predictions.  The combine runs in the inputs' dtype (float64 inputs: all float64; the fp32
    oracle's tensors: the oracle's own arithmetic, so phi = 0 restates it exactly), the rescale statistics always in float64"""
    e = eu + g * (ec - eu)
    if phi > 0.0:
        e = (e.double() * rescale_factor(e, ec, phi)).to(e.dtype)
    return e


def sched_reference(sch, eps_seq, table, phi, lat0, generator=None):
    """the loop of test_scheduler_ext_device_vs_mirror with the per-evaluation combine.  sch: a scheduler mirror with set_timesteps done;
    eps_seq: [evals, 2B, 4, h, w] ([uncond ; cond] per evaluation; the uncond half of a cond-only evaluation is never touched, it may hold
    NaN); table: one scale per evaluation; lat0 [B, 4, h, w]; generator: for the schedulers whose step() draws noise"""
    B = lat0.shape[0]
    x = lat0.double()
    extra = {} if generator is None else {"generator": generator}
    assert len(table) == len(sch.timesteps) == eps_seq.shape[0]
    for i, t in enumerate(sch.timesteps):
        ec = eps_seq[i, B:].double()
        e = guided_eps(eps_seq[i, :B].double(), ec, table[i], phi) if is_cfg(table[i]) else ec
        x = sch.step(e, t, x, **extra).prev_sample
    return x


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, table, phi=0.0, num_inference_steps=50, scheduler="ddim",
                    cloth_cond_rate=1.0, no_pose=False, int_layers=(1, 2, 3, 4, 5), trace=None, counts=None):
    """oracle/pipeline.py tryon_pipeline (lines 210-287) restated with a per-evaluation scale `table` (one entry per scheduler timestep), the
    combine above, and a UNet forward over the B conditional samples alone on cond-only evaluations of a CFG run.  counts (a dict) receives
    how many forwards ran over 2B and over B samples."""
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    do_cfg = any(is_cfg(g) for g in table)
    sf = vae_cfg["scaling_factor"]
    pe_c = inp["prompt_embeds"]
    pe = torch.cat([inp["negative_prompt_embeds"], pe_c]) if do_cfg else pe_c
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
    sch = P.make_scheduler(scheduler)
    sch.set_timesteps(num_inference_steps)
    assert len(table) == len(sch.timesteps), (len(table), len(sch.timesteps))
    cloth_conditioning_steps = (1 - cloth_cond_rate) * num_inference_steps
    latents = inp["noise_latents"] * sch.init_noise_sigma
    h, w = image.shape[2] // 8, image.shape[3] // 8
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
        masked_lat_in = torch.cat([masked_lat] * 2)
        pose = torch.cat([torch.zeros_like(pose), pose])
        if cloth_latents is not None:
            cloth_latents = torch.cat([torch.zeros_like(cloth_latents), cloth_latents])
    else:
        masked_lat_in = masked_lat
    if trace is not None:
        trace.update(noise_pred=[], latents=[])
    n_full = n_cond = 0
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and is_cfg(table[i])
        x = torch.cat([latents] * 2) if cfg_i else latents
        if cloth_latents is not None and i >= (num_inference_steps - cloth_conditioning_steps):
            cloth_latents = torch.zeros_like(cloth_latents)
        x = sch.scale_model_input(x, t)
        parts = [mask_lat, masked_lat_in, pose] + ([cloth_latents] if cloth_latents is not None else [])
        if do_cfg and not cfg_i:
            parts = [p[B:] for p in parts]        # the conditional half of every static input, the conditional context
        x = torch.cat([x] + parts, dim=1)
        eps = M.unet_forward(unet_sd, unet_cfg, x, t, pe if cfg_i or not do_cfg else pe_c)
        if cfg_i:
            eu, et = eps.chunk(2)
            eps = guided_eps(eu, et, table[i], phi)
            n_full += 1
        else:
            n_cond += 1
        latents = sch.step(eps, t, latents)
        if trace is not None:
            trace["noise_pred"].append(eps)
            trace["latents"].append(latents)
    if counts is not None:
        counts.update(full=n_full, cond_only=n_cond)
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
