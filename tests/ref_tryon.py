"""The one reference try-on loop the test oracles share: oracle/pipeline.py tryon_pipeline restated over tests/ref_unet.py's forward, with
every option the fused loop has.  Each feature's own mathematics stays in its module (guidance_ref, strength_ref, preserve_ref, pag_ref,
ip_adapter_ref, feature_cache_ref.plan); this module only says where in the loop it acts.  With the oracle's own scheduler, a constant
guidance table and every other option off it is tryon_pipeline bit for bit (tests/test_cpu_guidance.py asserts it).

    scheduler       a name of strength_ref.SCHEDULERS: the package's mirror (strength_ref.make_mirror), or a ready scheduler object with
                    set_timesteps / timesteps / init_noise_sigma / scale_model_input / step, such as oracle.pipeline.make_scheduler's, whose
                    step returns the tensor itself
    guidance, table one scale for all evaluations, or one per evaluation of the run; an evaluation with g <= 1 of a CFG run runs over the
                    conditional samples alone.  phi: guidance rescale
    pag             (scale, adaptive scale, `pag_applied_layers` names): an evaluation with s_i > 0 has a perturbed sample group
    ip              (sd_ip, embeds [B, E], negative embeds or None = zeros, scales per block): the uncond group gets image_proj(negative), the
                    cond and the perturbed group image_proj(embeds)
    freeu           (s1, s2, b1, b2)
    feature_cache   (interval, branch): interval None (every evaluation whole and nothing captured), an int or one flag per evaluation;
                    feature_cache_ref.plan gives the flags after promotion.  A whole evaluation refreshes the cache rows of the samples it ran
                    over (one row per sample of the context batch [uncond ; cond]), a shallow one reads them
    init_latents, first_step, init_is_noisy     the start at step first_step of the schedule (strength_ref); first_step = 0 ignores the init
    preserve        (mode, feather_sigma), mode None / "latents" / "pixels" / "both": the latent blend after every scheduler step, the
                    composite after the decode (preserve_ref)
    cloth_cond_rate the pipeline's rule: evaluation i sees zero cloth latents from i >= tail - (1 - rate) * tail on, tail the number of steps
                    run.  At rate 1 that still is PNDM's extra evaluation (i = tail), as in oracle.pipeline.tryon_pipeline and in the library.
                    None: no cut-off at all, what the PAG and image-prompt end-to-end tests have compared their PNDM case with so far
    tome            (tcfg, forced_per_eval): forced_per_eval None, or per evaluation a dict prefix -> a plan per sample of its batch
    callback        callback(i, latents) -> latents after every evaluation (after the blend)
    info            a dict that receives full / cond_only / shallow / pag / evals (counts of evaluations), flags (the promoted cache plan or
                    None), pag_table, noise_pred and latents (per evaluation: the combined prediction, the latents it leaves) and seen
                    ((i, t) per evaluation)

The batch of an evaluation is [uncond?] + [cond] * (1 or 2) sample groups, with context, image tokens and cache rows row for row.
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from tests import feature_cache_ref as FC
from tests import guidance_ref as G
from tests import ip_adapter_ref as IP
from tests import pag_ref as PG
from tests import preserve_ref as PR
from tests import ref_unet as RU
from tests import strength_ref as SR


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, *, guidance=7.5, table=None, phi=0.0,
                    pag=None, ip=None, freeu=None, feature_cache=None, init_latents=None, first_step=0, init_is_noisy=False, preserve=None,
                    tome=None, cloth_cond_rate=1.0, no_pose=False, generator=None, int_layers=(1, 2, 3, 4, 5), callback=None, info=None):
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    B = image.shape[0]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler) if isinstance(scheduler, str) else scheduler
    sch.set_timesteps(num_inference_steps, first_step=first_step) if first_step else sch.set_timesteps(num_inference_steps)
    n = len(sch.timesteps)
    table = [float(guidance)] * n if table is None else list(table)
    assert len(table) == n, (len(table), n)
    do_cfg = any(G.is_cfg(g) for g in table)
    ptab = PG.pag_plan(*pag[:2], sch.timesteps) if pag is not None else [0.0] * n
    sel = PG.layer_prefixes(pag[2], unet_cfg["layers_per_block"]) if pag is not None else set()
    interval, branch = feature_cache if feature_cache is not None else (None, 0)
    flags = FC.plan(n, interval, [do_cfg and not G.is_cfg(g) for g in table]) if interval is not None else None
    assert flags is None or not any(s > 0.0 for s in ptab), "the library refuses pag_scale > 0 with a feature cache"
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
    cache = None                      # [2B or B, C, h, w]: one row per sample of the context batch
    rows_c = slice(B, 2 * B) if do_cfg else slice(0, B)
    n_full = n_cond = n_shallow = n_pag = 0
    noise_pred, lat_seq, seen = [], [], []
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        pag_i = ptab[i] > 0.0
        if cloth_latents is not None and i >= cloth_off_from:
            cloth_latents = torch.zeros_like(cloth_latents)
        xs = sch.scale_model_input(latents, t)
        opt = [cloth_latents] if cloth_latents is not None else []
        x_c = torch.cat([xs, mask_lat, masked_lat, pose] + opt, dim=1)
        x_u = torch.cat([xs, mask_lat, masked_lat, torch.zeros_like(pose)] + [torch.zeros_like(c) for c in opt], dim=1)
        reps = 2 if pag_i else 1
        x = torch.cat(([x_u] if cfg_i else []) + [x_c] * reps)
        ehs = torch.cat(([pe_u] if cfg_i else []) + [pe_c] * reps)
        rows = slice(0, 2 * B) if cfg_i else rows_c
        kw = dict(freeu=freeu, pag=(sel, x.shape[0] - B) if pag_i else None)
        if ip is not None:
            kw["ip"] = (sd_ip, torch.cat(([tok_u] if cfg_i else []) + [tok_c] * reps), scales)
        if tome is not None:
            kw["tome"] = (tome[0], tome[1][i] if tome[1] is not None else None, None, "proj_in")
        if flags is None:
            eps = RU.unet_forward(unet_sd, unet_cfg, x, t, ehs, **kw)
        elif flags[i]:
            eps, cap = RU.unet_forward(unet_sd, unet_cfg, x, t, ehs, cache=("capture", branch), **kw)
            if cache is None:
                cache = torch.full(((2 * B if do_cfg else B),) + tuple(cap.shape[1:]), float("nan"))
            cache[rows] = cap
        else:
            eps = RU.unet_forward(unet_sd, unet_cfg, x, t, ehs, cache=("shallow", branch, cache[rows]), **kw)
            n_shallow += 1
        parts = list(eps.chunk(x.shape[0] // B))
        ep = parts.pop() if pag_i else None
        ec = parts.pop()
        eu = parts.pop() if cfg_i else None
        eps = PG.guided_eps(eu, ec, ep, table[i], ptab[i], phi)
        out = sch.step(eps, t, latents, **extra)
        latents = out if torch.is_tensor(out) else out.prev_sample
        if bits & 1:
            latents = PR.blend(latents, keep, z0, inp["noise_latents"], *kc[i])
        if callback is not None:
            latents = callback(i, latents)
        n_full += 1 if cfg_i else 0
        n_cond += 0 if cfg_i else 1
        n_pag += 1 if pag_i else 0
        noise_pred.append(eps)
        lat_seq.append(latents)
        seen.append((i, float(t)))
    if info is not None:
        info.update(full=n_full, cond_only=n_cond, shallow=n_shallow, pag=n_pag, evals=n, flags=flags, pag_table=ptab, noise_pred=noise_pred,
                    latents=lat_seq, seen=seen)
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    if bits & 2:
        img = PR.composite(img, image, PR.feather(mask, feather_sigma) if feather_sigma > 0 else mask).float()
    else:
        img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
