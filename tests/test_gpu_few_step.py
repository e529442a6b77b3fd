"""Few-step sampling on the device: LCM, TCD and trailing spacing through the fused step kernel (ladi_op_sched_run_noise[_eta]) against the
host mirrors, the tiny model end to end (fused hipGraph, fused eager, modular) against the oracle pipeline running the float64 restatement
of tests/few_step_ref.py, a run of ONE evaluation together with every per-evaluation feature of the fused loop, and the captured graphs of
one handle across scheduler codes that differ only in an option bit or in eta."""
import ctypes

import numpy as np
import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import few_step_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

F32 = lambda v: float(np.float32(v))          # noqa: E731  (eta as the C ABI carries it)
# name -> (mirror, restatement(noise_fn), eta)
KINDS = {
    "lcm": (lambda L: L.LCMScheduler(), lambda nf: R.RefLCM(noise_fn=nf), 0.0),
    "lcm_o100": (lambda L: L.LCMScheduler(original_inference_steps=100), lambda nf: R.RefLCM(original_steps=100, noise_fn=nf), 0.0),
    "tcd": (lambda L: L.TCDScheduler(), lambda nf: R.RefTCD(gamma=F32(0.3), noise_fn=nf), 0.3),
    "tcd_eta0": (lambda L: L.TCDScheduler(), lambda nf: R.RefTCD(gamma=0.0, noise_fn=nf), 0.0),
    "ddim_t": (lambda L: L.DDIMScheduler(timestep_spacing="trailing"), lambda nf: R.RefDDIM(eta=0.0, noise_fn=nf), 0.0),
    "ddim_t_eta": (lambda L: L.DDIMScheduler(timestep_spacing="trailing"), lambda nf: R.RefDDIM(eta=0.5, noise_fn=nf), 0.5),
    "euler_t": (lambda L: L.EulerDiscreteScheduler(timestep_spacing="trailing"), lambda nf: R.RefEuler(noise_fn=nf), 0.0),
    "euler_a_t": (lambda L: L.EulerAncestralDiscreteScheduler(timestep_spacing="trailing"), lambda nf: R.RefEuler(ancestral=True, noise_fn=nf), 0.0),
    "ddim": (lambda L: L.DDIMScheduler(), None, 0.0),
    "euler_a": (lambda L: L.EulerAncestralDiscreteScheduler(), None, 0.0),
}


def _mirror(kind):
    import ladi_vton_amd as L
    return KINDS[kind][0](L)


def _step_kw(kind):
    return {"eta": KINDS[kind][2]} if kind.startswith(("tcd", "ddim")) else {}


# ------------------------------------------------------------------------------------------------------------------ step kernel
@pytest.mark.parametrize("shape", [(2, 8, 12), (3, 9, 13)])
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["lcm", "tcd", "ddim_t", "ddim_t_eta", "euler_t", "euler_a_t"])
def test_few_step_device_vs_mirror(lib, kind, steps, cfg, shape):
    """fused CFG + scheduler update on the device vs the host mirror over the same random eps sequence and the same per-step noise; rel-L2 <
    1e-5 as test_scheduler_ext_device_vs_mirror.  Every slab the mirror does not draw for (the last of LCM and TCD) is NaN on the device:
    a finite result is the proof that it is never read"""
    sch, eta = _mirror(kind), KINDS[kind][2]
    sch.set_timesteps(steps)
    B, h, w = shape
    gs = 7.5 if cfg else 1.0
    hw = h * w
    rows = (2 if cfg else 1) * B
    g = torch.Generator().manual_seed(61)
    eps = torch.randn((steps, rows, hw, 4), generator=g).half()
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    gen, gen_dev = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
    x = lat0.clone()
    slabs = []
    for i, t in enumerate(sch.timesteps):
        e = eps[i].float().view(rows, h, w, 4).permute(0, 3, 1, 2)
        if cfg:
            e = e[:B] + gs * (e[B:] - e[:B])
        before = gen.get_state()
        x = sch.step(e, t, x, generator=gen, **_step_kw(kind)).prev_sample
        drew = not torch.equal(gen.get_state(), before)
        slabs.append(torch.randn((B, 4, h, w), generator=gen_dev) if drew else torch.full((B, 4, h, w), float("nan")))
    if kind in ("lcm", "tcd"):
        assert bool(torch.isnan(slabs[-1]).all()) and all(bool(torch.isfinite(s).all()) for s in slabs[:-1])
    E = eps.to(U.dev())
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = torch.stack(slabs).contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    if eta:
        rc = lib.ladi_op_sched_run_noise_eta(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), eta, ptr(E), steps, B, hw, cfg, gs, ptr(L_), ptr(N),
                                             steps, stream_ptr())
    else:
        rc = lib.ladi_op_sched_run_noise(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), ptr(E), steps, B, hw, cfg, gs, ptr(L_), ptr(N), steps,
                                         stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = L_.cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all())
    assert U.rel_l2(got, x) < 1e-5, U.rel_l2(got, x)


@pytest.mark.parametrize("kind", ["lcm", "tcd"])
def test_few_step_device_needs_noise(lib, kind):
    """no silent zero: a stochastic run without per-step noise, or with steps - 1 slabs of it, is an error (nothing is launched); a run of one
    evaluation has no stochastic term and needs none"""
    B, hw, steps = 1, 16, 4
    code, eta = _mirror(kind).kind, 0.3 if kind == "tcd" else 0.0
    E = torch.zeros((steps, B, hw, 4), dtype=torch.float16, device=U.dev())
    L_ = torch.zeros((B, hw, 4), device=U.dev())
    N = torch.zeros((steps, B, 4, hw), device=U.dev())
    run = lib.ladi_op_sched_run_noise_eta
    assert run(code, steps, None, eta, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), None, 0, stream_ptr()) < 0
    assert "noise" in _lib.last_error()
    assert run(code, steps, None, eta, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), ptr(N), steps - 1, stream_ptr()) < 0
    assert "noise" in _lib.last_error()
    assert run(code, steps, None, eta, ptr(E), steps, B, hw, 0, 1.0, ptr(L_), ptr(N), steps, stream_ptr()) == 0, _lib.last_error()
    assert run(code, 1, None, eta, ptr(E), 1, B, hw, 0, 1.0, ptr(L_), None, 0, stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, inp={}, fresh={})


TINY_CASES = {"lcm_4": ("lcm", 4), "lcm_1": ("lcm", 1), "tcd_4": ("tcd", 4), "euler_t_1": ("euler_t", 1), "ddim_t_3": ("ddim_t", 3)}
SEED = 77


def _inputs(tiny, size=(256, 192)):
    if size not in tiny["inp"]:
        inp = P.synthetic_inputs(2, size[0], size[1], L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny["inp"][size] = inp
    return tiny["inp"][size]


def _oracle(tiny, case, monkeypatch):
    if case not in tiny["ref"]:
        kind, steps = TINY_CASES[case]
        g = torch.Generator().manual_seed(SEED)
        ref = KINDS[kind][1](lambda shape: torch.randn(shape, generator=g))
        monkeypatch.setattr(P, "make_scheduler", lambda _kind: ref)
        tiny["ref"][case] = P.tryon_pipeline(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], _inputs(tiny),
                                             num_inference_steps=steps, guidance_scale=7.5, scheduler="restated")
    return tiny["ref"][case]


def _pipe(tiny, kind):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=_mirror(kind), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _run(tiny, kind, steps, fused=True, graph=True, pipe=None, seed=SEED, size=(256, 192), **kw):
    """one pipeline call -> (images, latents); `kind` replaces the scheduler of a given pipeline (same handle, another code)"""
    inp, d = _inputs(tiny, size), U.dev()
    if pipe is None:
        pipe = _pipe(tiny, kind)
    else:
        pipe.scheduler = _mirror(kind)
    kw.setdefault("guidance_scale", 7.5)
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=size[0], width=size[1], num_inference_steps=steps,
               eta=KINDS[kind][2], output_type="np", fused=fused, use_graph=graph, generator=torch.Generator().manual_seed(seed),
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _same(a, b):
    """the tiny thresholds of test_tryon_pipeline_tiny: latents >= 40 dB, image >= 35 dB on [0, 1]"""
    p_img, p_lat = U.psnr(a[0], b[0], peak=1.0), U.psnr(a[1], b[1])
    assert a[0].shape == b[0].shape
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


@pytest.mark.parametrize("fused,graph", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("case", list(TINY_CASES))
def test_tryon_pipeline_tiny_few_step(tiny, case, fused, graph, monkeypatch):
    """end to end vs the oracle pipeline with the restated scheduler; a seeded CPU generator on both sides supplies the per-step noise"""
    ref = _oracle(tiny, case, monkeypatch)
    _same(_run(tiny, *TINY_CASES[case], fused=fused, graph=graph), ref)


@pytest.mark.parametrize("case", ["lcm_4", "tcd_4"])
def test_few_step_fused_equals_modular_same_seed(tiny, case):
    """the fused path's evaluations - 1 up-front draws are the modular path's per-step draws: same seed, same result"""
    kind, steps = TINY_CASES[case]
    f, m = _run(tiny, kind, steps, True, True), _run(tiny, kind, steps, False, False)
    _same(f, m)
    if case == "lcm_4":
        # a different seed gives a visibly different result: the comparison above does see the noise
        other = _run(tiny, kind, steps, True, True, seed=SEED + 1)
        assert U.psnr(other[1], f[1]) < 30.0
        # and the fused loop refuses to run LCM without its noise
        pipe, inp, d = _pipe(tiny, kind), _inputs(tiny), U.dev()
        with pytest.raises(_lib.NativeError, match="noise"):
            pipe._run_fused(inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
                            inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], 256, 192, 4, 7.5,
                            1.0, False, True, step_noise=None)


# ------------------------------------------------------------------------------------------------------------------ one evaluation
ONE_EVAL = {
    "preserve": dict(preserve_unmasked="both"),
    "feature_cache": dict(feature_cache=2),
    "pag": dict(pag_scale=2.0),
    "guidance_list": dict(guidance_scale=[1.0]),
    "plain_no_cfg": dict(guidance_scale=1.0),
}


@pytest.mark.parametrize("name", list(ONE_EVAL))
def test_one_evaluation_run_with_a_feature_on(tiny, name):
    """LCM, one step: the fused loop (use_graph asked for) completes with every per-evaluation feature and equals the modular path"""
    pipe = _pipe(tiny, "lcm")
    f = _run(tiny, "lcm", 1, True, True, pipe=pipe, **ONE_EVAL[name])
    assert bool(torch.isfinite(f[1]).all())
    if name in ("guidance_list", "plain_no_cfg"):
        assert pipe.cond_only_evals() == 1
    _same(f, _run(tiny, "lcm", 1, False, False, **ONE_EVAL[name]))


def test_one_evaluation_run_with_an_image_prompt(tiny):
    """IP-Adapter on a UNet of its own (the module's shared one stays plain): one LCM step, fused equals modular, and the prompt is seen"""
    import ladi_vton_amd as L
    from tests import ip_adapter_ref as IR
    unet = L.NativeUNet(tiny["ucfg"], tiny["sd"]["unet"])
    unet.load_ip_adapter(IR.to_diffusers(IR.make_adapter(tiny["ucfg"], 4, 64), 2, numbered=True))
    unet.set_ip_adapter_scale(1.0)
    emb = torch.randn((2, 64), generator=torch.Generator().manual_seed(5)).half().float().to(U.dev())

    def pipe():
        return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=unet, scheduler=_mirror("lcm"),
                                               emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])
    f = _run(tiny, "lcm", 1, True, True, pipe=pipe(), ip_adapter_image_embeds=emb)
    _same(f, _run(tiny, "lcm", 1, False, False, pipe=pipe(), ip_adapter_image_embeds=emb))
    assert not torch.equal(f[1], _run(tiny, "lcm", 1, True, True)[1])


def test_one_evaluation_run_callback(tiny):
    seen, seen_m = [], []
    f = _run(tiny, "lcm", 1, True, True, callback=lambda i, t, x: seen.append((i, int(t), tuple(x.shape))))
    m = _run(tiny, "lcm", 1, False, False, callback=lambda i, t, x: seen_m.append((i, int(t), tuple(x.shape))))
    assert seen == seen_m == [(0, 999, (2, 4, 32, 24))]
    _same(f, m)


def test_one_evaluation_tail_of_a_four_step_run(tiny):
    """strength 0.25 of 4 steps: first_step = 3, one evaluation at t = 259 from k_x init + k_n noise"""
    init = torch.randn((2, 4, 32, 24), generator=torch.Generator().manual_seed(3))
    seen = []
    f = _run(tiny, "lcm", 4, True, True, strength=0.25, init_latents=init, callback=lambda i, t, x: seen.append((i, int(t))))
    assert seen == [(0, 259)]
    _same(f, _run(tiny, "lcm", 4, False, False, strength=0.25, init_latents=init))
    one = _run(tiny, "lcm", 1, True, True)
    assert U.psnr(f[1], one[1]) < 30.0                           # not the one-step run from noise at t = 999


# ------------------------------------------------------------------------------------------------------------------ graphs of one handle
SMALL = (64, 48)
SEQUENCE = [("lcm", 4), ("tcd", 4), ("tcd_eta0", 4), ("lcm_o100", 4), ("ddim_t", 4), ("ddim", 4), ("lcm", 4)]


def _fresh(tiny, kind, steps):
    if (kind, steps) not in tiny["fresh"]:
        tiny["fresh"][(kind, steps)] = _run(tiny, kind, steps, True, True, size=SMALL)
    return tiny["fresh"][(kind, steps)]


def test_no_stale_graph_across_option_bits_and_eta(tiny):
    """ONE handle with use_graph runs codes that differ only in the kind, in original_inference_steps, in the trailing bit or in TCD's eta:
    each result is bit-equal to the same run on a fresh handle (nobody replays another run's table), and neighbours differ"""
    pipe = _pipe(tiny, "lcm")
    got = [_run(tiny, kind, steps, True, True, pipe=pipe, size=SMALL) for kind, steps in SEQUENCE]
    for (kind, steps), g in zip(SEQUENCE, got):
        want = _fresh(tiny, kind, steps)
        assert torch.equal(g[1], want[1]) and torch.equal(g[0], want[0]), kind
    for a, b in zip(got, got[1:]):
        assert not torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["ddim", "euler_a"])
def test_plain_runs_untouched_by_an_earlier_few_step_run(tiny, kind):
    """a plain 6-step run gives the same bits with and without an earlier LCM run on the same handle"""
    want = _fresh(tiny, kind, 6)
    pipe = _pipe(tiny, "lcm")
    _run(tiny, "lcm", 4, True, True, pipe=pipe, size=SMALL)
    got = _run(tiny, kind, 6, True, True, pipe=pipe, size=SMALL)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
