"""DPM-Solver++ multistep, Euler and Euler-ancestral on the device: the fused step kernel (ladi_op_sched_run_noise) vs the host mirrors,
the tiny model end to end (fused hipGraph, fused eager, modular) and the full-size model (DPM++ 2M, 25 steps) against the oracle
pipeline running the test-local float64 restatement (tests/sched_ext_ref.py) in place of its own schedulers."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import sched_ext_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

DPM_CASES = [(1, "midpoint", True), (2, "midpoint", True), (2, "heun", True), (3, "midpoint", True), (3, "heun", False), (2, "midpoint", False)]


def _mirror(kind):
    import ladi_vton_amd as L
    if kind == "euler":
        return L.EulerDiscreteScheduler()
    if kind == "euler_a":
        return L.EulerAncestralDiscreteScheduler()
    order, solver_type, lof = kind
    return L.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type, lower_order_final=lof)


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("steps", [8, 20])
@pytest.mark.parametrize("kind", DPM_CASES + ["euler", "euler_a"])
def test_scheduler_ext_device_vs_mirror(lib, kind, steps, cfg):
    """fused CFG + scheduler update on the device vs the host mirror over a random eps sequence (and, for Euler-ancestral, the same
    per-step noise the mirror draws from its generator); rel-L2 < 1e-5 as for DDIM / PNDM in test_scheduler_device_vs_oracle"""
    sch = _mirror(kind)
    sch.set_timesteps(steps)
    B, h, w, gs = 2, 8, 12, 7.5 if cfg else 1.0
    hw = h * w
    rows = (2 if cfg else 1) * B
    g = torch.Generator().manual_seed(61)
    eps = torch.randn((steps, rows, hw, 4), generator=g).half()
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    gen, gen_dev = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
    x = lat0.clone()
    for i, t in enumerate(sch.timesteps):
        e = eps[i].float().view(rows, h, w, 4).permute(0, 3, 1, 2)
        if cfg:
            e = e[:B] + gs * (e[B:] - e[:B])
        x = sch.step(e, t, x, generator=gen).prev_sample
    noise = torch.stack([torch.randn((B, 4, h, w), generator=gen_dev) for _ in range(steps)]).contiguous()
    E = eps.to(U.dev())
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = noise.to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    rc = lib.ladi_op_sched_run_noise(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), ptr(E), steps, B, hw, cfg, gs, ptr(L_), ptr(N), steps,
                                     stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = L_.cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    assert U.rel_l2(got, x) < 1e-5, U.rel_l2(got, x)


def test_euler_ancestral_device_needs_noise(lib):
    """no silent zero: Euler-ancestral without per-step noise, or with too few steps of it, is an error (nothing is launched)"""
    B, hw, steps = 1, 16, 5
    E = torch.zeros((steps, B, hw, 4), dtype=torch.float16, device=U.dev())
    L_ = torch.zeros((B, hw, 4), device=U.dev())
    N = torch.zeros((steps, B, 4, hw), device=U.dev())
    assert lib.ladi_op_sched_run_noise(5, steps, None, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), None, 0, stream_ptr()) < 0
    assert "noise" in _lib.last_error()
    assert lib.ladi_op_sched_run_noise(5, steps, None, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), ptr(N), steps - 1, stream_ptr()) < 0
    assert lib.ladi_op_sched_run(5, steps, None, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), stream_ptr()) < 0


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={})


TINY_CASES = {"dpmpp2m_6": ((2, "midpoint", True), 6), "dpmpp2m_20": ((2, "midpoint", True), 20), "dpm_order3": ((3, "midpoint", True), 8),
              "dpm_heun": ((2, "heun", True), 8), "euler": ("euler", 7), "euler_a": ("euler_a", 7)}
SEED = 77


def _restatement(kind):
    if kind == "euler":
        return R.RefEuler()
    if kind == "euler_a":
        g = torch.Generator().manual_seed(SEED)
        return R.RefEuler(ancestral=True, noise_fn=lambda shape: torch.randn(shape, generator=g))
    return R.RefDPM(*kind)


def _tiny_inputs(tiny):
    B, H, W, L_, D = 2, 256, 192, 8, tiny["ucfg"]["cross_attention_dim"]
    inp = P.synthetic_inputs(B, H, W, L=L_, D=D)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp, H, W


def _tiny_oracle(tiny, case, monkeypatch):
    if case not in tiny["ref"]:
        kind, steps = TINY_CASES[case]
        inp, H, W = _tiny_inputs(tiny)
        monkeypatch.setattr(P, "make_scheduler", lambda _kind: _restatement(kind))
        tiny["ref"][case] = P.tryon_pipeline(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp,
                                             num_inference_steps=steps, guidance_scale=7.5, scheduler="restated")
    return tiny["ref"][case]


def _tiny_run(tiny, case, fused, graph, pipe=None):
    import ladi_vton_amd as L
    kind, steps = TINY_CASES[case]
    inp, H, W = _tiny_inputs(tiny)
    pipe = pipe or L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                                   scheduler=_mirror(kind), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=steps,
               guidance_scale=7.5, output_type="np", fused=fused, use_graph=graph, generator=torch.Generator().manual_seed(SEED),
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


@pytest.mark.parametrize("fused,graph", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("case", list(TINY_CASES))
def test_tryon_pipeline_tiny_scheduler_ext(tiny, case, fused, graph, monkeypatch):
    """end to end vs the oracle pipeline with the restated scheduler; thresholds of test_tryon_pipeline_tiny (latents >= 40 dB, image
    >= 35 dB on [0,1]).  Euler-ancestral: a seeded CPU generator on both sides supplies the per-step noise."""
    ref_img, ref_lat = _tiny_oracle(tiny, case, monkeypatch)
    img, lat = _tiny_run(tiny, case, fused, graph)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    assert img.shape == ref_img.shape
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


def test_euler_ancestral_fused_equals_modular_same_seed(tiny):
    """the fused path's up-front draws are the modular path's per-step draws: same seed, same result"""
    img_f, lat_f = _tiny_run(tiny, "euler_a", True, True)
    img_m, lat_m = _tiny_run(tiny, "euler_a", False, False)
    assert U.psnr(lat_f, lat_m) >= 40.0 and U.psnr(img_f, img_m, peak=1.0) >= 35.0, (U.psnr(lat_f, lat_m), U.psnr(img_f, img_m, peak=1.0))
    # a different seed gives a visibly different result: the comparison above does see the noise
    import ladi_vton_amd as L
    inp, H, W = _tiny_inputs(tiny)
    pipe = L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=L.EulerAncestralDiscreteScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])
    d = U.dev()
    pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
         warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
         negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=TINY_CASES["euler_a"][1],
         guidance_scale=7.5, output_type="np", generator=torch.Generator().manual_seed(SEED + 1),
         noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    assert U.psnr(pipe.last_latents.float().cpu(), lat_f) < 30.0
    # and the fused loop refuses to run Euler-ancestral without its noise
    with pytest.raises(_lib.NativeError, match="noise"):
        pipe._run_fused(inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
                        inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, 7, 7.5,
                        1.0, False, True, step_noise=None)


# ------------------------------------------------------------------------------------------------------------------ full-size model
def test_dpmpp_2m_25_steps_full_vs_oracle():
    """DPM++ 2M, 25 steps, B = 1, 512x384, EMASC on, fused hipGraph loop vs the oracle (restated scheduler); guards of
    test_baseline_config_50_steps_vs_oracle: image >= 60 dB, final latents >= 62 dB, guided noise_pred >= 52 dB, uint8 max diff <= 2"""
    import ladi_vton_amd as L
    torch.set_num_threads(U.cpu_quota_threads())
    ucfg, vcfg, ecfg = C.UNET_FULL, C.VAE_FULL, C.EMASC_FULL
    sd = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
              emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    B, H, W, steps = 1, 512, 384, 25
    inp = P.synthetic_inputs(B, H, W, L=77, D=1024)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    trace = {}
    orig = P.make_scheduler
    P.make_scheduler = lambda _kind: R.RefDPM(2, "midpoint", True)
    try:
        ref_img, ref_lat = P.tryon_pipeline(sd["unet"], ucfg, sd["vae"], vcfg, sd["emasc"], inp, num_inference_steps=steps, guidance_scale=7.5,
                                            scheduler="restated", trace=trace)
    finally:
        P.make_scheduler = orig
    pipe = L.StableDiffusionTryOnePipeline(vae=L.NativeVAE(vcfg, sd["vae"]), text_encoder=None, tokenizer=None, unet=L.NativeUNet(ucfg, sd["unet"]),
                                           scheduler=L.DPMSolverMultistepScheduler(), emasc=L.NativeEMASC(ecfg, sd["emasc"]),
                                           emasc_int_layers=[1, 2, 3, 4, 5])
    pipe.trace_evals = steps
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=steps,
               guidance_scale=7.5, output_type="np", fused=True, use_graph=True,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    img = torch.from_numpy(out.images)
    lat = pipe.last_latents.float().cpu()
    tr = {k: v.cpu() for k, v in pipe.last_trace.items()}
    assert len(trace["noise_pred"]) == steps
    eps_psnr = [round(U.psnr(tr["noise_pred"][i], trace["noise_pred"][i]), 2) for i in range(steps)]
    u8a, u8b = (img * 255).round(), (ref_img * 255).round()
    res = dict(image_psnr_db=round(U.psnr(img, ref_img, 1.0), 2), final_latents_psnr_db=round(U.psnr(lat, ref_lat), 2),
               uint8_max_abs_diff=int((u8a - u8b).abs().max()), noise_pred_psnr_db_min=min(eps_psnr), noise_pred_psnr_db_per_eval=eps_psnr)
    U.record_parity("tryon_512x384_25_dpmpp2m_B1", res)
    assert img.shape == ref_img.shape == (B, H, W, 3)
    assert torch.equal(tr["latents"][-1], lat)
    assert res["image_psnr_db"] >= 60.0, res
    assert res["final_latents_psnr_db"] >= 62.0 and res["noise_pred_psnr_db_min"] >= 52.0, res
    assert res["uint8_max_abs_diff"] <= 2, res
