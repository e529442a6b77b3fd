"""Reference for the deep-feature cache (DeepCache on the full-resolution level): the yardstick tests/test_cpu_feature_cache.py and
tests/test_gpu_feature_cache.py compare the library with.  The UNet forward is composed from oracle.models' block functions the way
tests/anysize_ref.py composes its own (so it also runs latent sizes that are no multiple of 8); the loop is tests/strength_ref.py's with a
plan.  Nothing here imports the package under test except its scheduler mirrors (as tests/strength_ref.py does).

Names are diffusers', L = layers_per_block.
    whole forward            oracle.models.unet_forward; with capture it also hands back the hidden state that enters
                             up_blocks.3.resnets.(L - k), before the concatenation with its skip: the output of up_blocks.3.attentions.(L - k - 1)
                             for k < L, of up_blocks.2.upsamplers.0 for k = L
    shallow forward, branch k conv_in, layers 0 .. k-1 of down_blocks.0 (skips 0 .. k), then up_blocks.3 layers L-k .. L, the first from the
                             cached tensor, conv_norm_out, conv_out; time embedding of the evaluation's own timestep
    plan                     one flag per evaluation, True = whole; flag 0 is whole.  Promotion: in a CFG-shaped run a shallow evaluation over
                             all 2B samples whose most recent whole evaluation ran cond-only (and so refreshed the conditional rows only) runs
                             whole; a shallow cond-only evaluation never does
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from tests import guidance_ref as G
from tests import strength_ref as SR


def unet_forward(sd, cfg, sample, timestep, ehs, mode=None, branch=0, cache=None):
    """mode None: the whole forward -> out.  "capture": the whole forward -> (out, cached tensor [n, boc[0], h, w]; boc[1] channels
    for branch = L, which caches the output of up_blocks.2's upsampler).  "shallow": the shallow
    forward from `cache` -> out.  One loop body for all three: a layer either runs or is skipped."""
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
            x = torch.cat([x, skips.pop()], dim=1)
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


def plan(n_evals, interval, cond_only=None):
    """-> [bool] * n_evals after promotion.  interval: an int N >= 1 (whole at i % N == 0) or a sequence of n_evals flags; cond_only: None or
    one flag per evaluation (True: that evaluation of a CFG-shaped run runs over the conditional samples alone)"""
    flags = [i % interval == 0 for i in range(n_evals)] if isinstance(interval, int) else [bool(f) for f in interval]
    assert len(flags) == n_evals
    co = [False] * n_evals if cond_only is None else [bool(c) for c in cond_only]
    if flags:
        flags[0] = True
    only_cond_rows_fresh = False
    for i in range(n_evals):
        if not flags[i] and not co[i] and only_cond_rows_fresh:
            flags[i] = True
        if flags[i]:
            only_cond_rows_fresh = co[i]
    return flags


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, interval, branch, num_inference_steps, scheduler, guidance=7.5,
                    table=None, init_latents=None, first_step=0, cloth_cond_rate=1.0, generator=None, int_layers=(1, 2, 3, 4, 5), counts=None):
    """tests/strength_ref.py tryon_reference (the oracle modules, the mirror scheduler `scheduler` over its evaluations, a per-evaluation
    guidance `table`, an optional start at first_step) with the plan above: a whole evaluation refreshes the cache rows of the samples it
    ran over, a shallow one reads them.  interval: None (the plain loop: oracle.models.unet_forward every evaluation), an int or a sequence of
    flags.  counts (a dict) receives shallow / cond_only / evals and the promoted flags."""
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
    flags = plan(n, interval, co) if interval is not None else None
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
    cache = None                      # [2B or B, C, h, w]: one row per sample of the context batch
    n_shallow = n_cond = 0
    for i, t in enumerate(sch.timesteps):
        cfg_i = do_cfg and G.is_cfg(table[i])
        x = torch.cat([latents] * 2) if cfg_i else latents
        if cloth_latents is not None and i >= (tail - cloth_conditioning_steps):
            cloth_latents = torch.zeros_like(cloth_latents)
        x = sch.scale_model_input(x, t)
        parts = [mask_lat, masked_lat, pose] + ([cloth_latents] if cloth_latents is not None else [])
        sub = do_cfg and not cfg_i     # the conditional samples alone: rows [B, 2B) of every per-sample thing
        if sub:
            parts = [p[B:] for p in parts]
        x = torch.cat([x] + parts, dim=1)
        ehs = pe_c if sub else pe
        rows = slice(B, 2 * B) if sub else slice(0, 2 * B if do_cfg else B)
        if flags is None:
            eps = M.unet_forward(unet_sd, unet_cfg, x, t, ehs)
        elif flags[i]:
            eps, cap = unet_forward(unet_sd, unet_cfg, x, t, ehs, "capture", branch)
            if cache is None:
                cache = torch.full(((2 * B if do_cfg else B),) + tuple(cap.shape[1:]), float("nan"))
            cache[rows] = cap
        else:
            eps = unet_forward(unet_sd, unet_cfg, x, t, ehs, "shallow", branch, cache[rows])
            n_shallow += 1
        n_cond += 0 if cfg_i else 1
        if cfg_i:
            eu, et = eps.chunk(2)
            eps = G.guided_eps(eu, et, table[i])
        latents = sch.step(eps, t, latents, **extra).prev_sample
    if counts is not None:
        counts.update(shallow=n_shallow, cond_only=n_cond, evals=n, flags=flags)
    z = latents / sf
    img = M.vae_decode(vae_sd, vae_cfg, z, list(inter) if inter is not None else None, list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
