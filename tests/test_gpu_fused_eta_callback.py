"""DDIM with eta > 0 and step callbacks on the fused loop: the step kernel with the eta table (ladi_op_sched_run_noise_eta) vs the float64
restatement (tests/ddim_eta_ref.py), and the tiny model end to end -- fused hipGraph, fused eager and modular against each other and against
the oracle pipeline fed the same draws -- plus what the callback sees, in-place edits, and an exception in the callback."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import ddim_eta_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

DDIM = 0


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_ddim_eta_device_vs_restatement(lib, eta, cfg):
    """fused CFG + DDIM-eta update on the device vs float64 over a random eps / noise sequence; rel-L2 < 1e-5 as for the other schedulers"""
    steps, B, h, w, gs = 10, 2, 8, 12, 7.5 if cfg else 1.0
    hw, rows = h * w, (2 if cfg else 1) * B
    g = torch.Generator().manual_seed(23)
    eps = torch.randn((steps, rows, hw, 4), generator=g).half()
    noise = torch.randn((steps, B, 4, h, w), generator=g)
    x = torch.randn((B, 4, h, w), generator=g).double()
    lat0 = x.float().permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous()
    for i in range(steps):
        e = eps[i].double().view(rows, h, w, 4).permute(0, 3, 1, 2)
        if cfg:
            e = e[:B] + gs * (e[B:] - e[:B])
        x = R.step(steps, i, eta, x, e, noise[i].double())
    E, L_, N = eps.to(U.dev()), lat0.to(U.dev()), noise.contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    rc = lib.ladi_op_sched_run_noise_eta(DDIM, steps, ctypes.c_void_p(ac.data_ptr()), eta, ptr(E), steps, B, hw, cfg, gs, ptr(L_), ptr(N),
                                         steps, stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = L_.cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    assert U.rel_l2(got, x) < 1e-5, U.rel_l2(got, x)
    # no silent zero: eta > 0 without noise is an error
    assert lib.ladi_op_sched_run_noise_eta(DDIM, steps, None, eta, ptr(E), steps, B, hw, cfg, gs, ptr(L_), None, 0, stream_ptr()) < 0
    assert "noise" in _lib.last_error()


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


SEED, STEPS = 91, 8


def _tiny_inputs(tiny):
    B, H, W, L_, D = 2, 256, 192, 8, tiny["ucfg"]["cross_attention_dim"]
    inp = P.synthetic_inputs(B, H, W, L=L_, D=D)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp, H, W


def _pipe(tiny, scheduler="ddim"):
    import ladi_vton_amd as L
    sch = L.DDIMScheduler() if scheduler == "ddim" else L.PNDMScheduler()
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"], scheduler=sch,
                                           emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _run(tiny, fused=True, graph=True, eta=0.0, seed=SEED, pipe=None, scheduler="ddim", steps=STEPS, **kw):
    inp, H, W = _tiny_inputs(tiny)
    pipe = pipe or _pipe(tiny, scheduler)
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=steps,
               guidance_scale=7.5, output_type="np", fused=fused, use_graph=graph, eta=eta, generator=torch.Generator().manual_seed(seed),
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


class _EtaDDIM(P.DDIM):
    """the oracle's DDIM with eta, fed one [B, 4, h, w] draw per step from a seeded CPU generator -- the draws the pipeline makes"""

    def __init__(self, eta, seed):
        super().__init__()
        self.eta, self.g = eta, torch.Generator().manual_seed(seed)

    def step(self, eps, t, x):
        return super().step(eps, t, x, eta=self.eta, noise=torch.randn(tuple(x.shape), generator=self.g))


def _oracle(tiny, eta, monkeypatch):
    if eta not in tiny["ref"]:
        inp, H, W = _tiny_inputs(tiny)
        monkeypatch.setattr(P, "make_scheduler", lambda _kind: _EtaDDIM(eta, SEED))
        tiny["ref"][eta] = P.tryon_pipeline(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp,
                                            num_inference_steps=STEPS, guidance_scale=7.5, scheduler="restated")
    return tiny["ref"][eta]


def _close(a, b):
    (img_a, lat_a), (img_b, lat_b) = a, b
    p_img, p_lat = U.psnr(img_a, img_b, peak=1.0), U.psnr(lat_a, lat_b)
    assert img_a.shape == img_b.shape
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_ddim_eta_fused_matches_modular_and_oracle(tiny, eta, monkeypatch):
    """same seed: fused hipGraph and fused eager each match the modular path and the oracle fed the same draws (latents >= 40 dB, image
    >= 35 dB); another seed moves the latents (< 30 dB), so the comparison does see the noise"""
    modular = _run(tiny, fused=False, graph=False, eta=eta)
    ref = _oracle(tiny, eta, monkeypatch)
    for graph in (True, False):
        fused = _run(tiny, graph=graph, eta=eta)
        _close(fused, modular)
        _close(fused, ref)
    _close(modular, ref)
    other = _run(tiny, eta=eta, seed=SEED + 1)
    assert U.psnr(other[1], modular[1]) < 30.0


def _no_modular(monkeypatch):
    import ladi_vton_amd as L

    def boom(*a, **k):
        raise AssertionError("the module-by-module path ran")
    monkeypatch.setattr(L.StableDiffusionTryOnePipeline, "_run_modular", boom)


def test_fused_path_taken_with_eta(tiny, monkeypatch):
    _no_modular(monkeypatch)
    img, lat = _run(tiny, eta=0.5)
    assert torch.isfinite(lat).all()


def test_fused_path_taken_with_callback(tiny, monkeypatch):
    _no_modular(monkeypatch)
    seen = []
    _run(tiny, callback=lambda i, t, x: seen.append(i))
    assert seen == list(range(STEPS))


def _record(tiny, fused, graph, scheduler, every, steps=STEPS):
    pipe = _pipe(tiny, scheduler)
    evals = steps + (1 if scheduler == "pndm" else 0)
    if fused:
        pipe.trace_evals = evals
    rec = []
    res = _run(tiny, fused=fused, graph=graph, pipe=pipe, scheduler=scheduler, steps=steps,
               callback=lambda i, t, x: rec.append((i, int(t), x.clone())), callback_steps=every)
    return rec, res, (pipe.last_trace if fused else None)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("scheduler", ["pndm", "ddim"])
def test_callback_contents(tiny, scheduler, every, graph):
    """the (i, t) sequence is the modular path's; each latents tensor is that evaluation of the per-evaluation trace, bit for bit"""
    rec_f, res_f, trace = _record(tiny, True, graph, scheduler, every)
    rec_m, res_m, _ = _record(tiny, False, False, scheduler, every)
    assert [(i, t) for i, t, _ in rec_f] == [(i, t) for i, t, _ in rec_m]
    assert len(rec_f) > 1
    for i, _, x in rec_f:
        assert x.dtype == torch.float32 and x.shape == trace["latents"][i].shape
        assert torch.equal(x, trace["latents"][i]), i
    for (_, _, xf), (_, _, xm) in zip(rec_f, rec_m):
        assert U.psnr(xf.cpu(), xm.cpu()) >= 40.0
    _close(res_f, res_m)


def test_callback_short_loop(tiny):
    """the loop form with fewer than three evaluations (no graph): callback at both, matching the modular path"""
    rec_f, res_f, _ = _record(tiny, True, True, "ddim", 1, steps=2)
    rec_m, res_m, _ = _record(tiny, False, False, "ddim", 1, steps=2)
    assert [(i, t) for i, t, _ in rec_f] == [(i, t) for i, t, _ in rec_m] and len(rec_f) == 2
    _close(res_f, res_m)


def _halve_at_2(i, t, x):
    if i == 2:
        x.mul_(0.5)


@pytest.mark.parametrize("scheduler", ["pndm", "ddim"])
def test_callback_in_place_edit(tiny, scheduler):
    """latents.mul_(0.5) at step 2 takes effect on the fused loop as on the modular path, and visibly changes the result"""
    plain = _run(tiny, scheduler=scheduler)
    for graph in (True, False):
        edited = _run(tiny, graph=graph, scheduler=scheduler, callback=_halve_at_2)
        _close(edited, _run(tiny, fused=False, graph=False, scheduler=scheduler, callback=_halve_at_2))
        assert U.psnr(edited[1], plain[1]) < 30.0


def test_callback_noop_is_bit_identical(tiny):
    """a callback that edits nothing changes no bit (export / import round trip, UNet input rewritten with the same rounding)"""
    plain = _run(tiny, scheduler="pndm")
    seen = _run(tiny, scheduler="pndm", callback=lambda i, t, x: None)
    assert torch.equal(plain[0], seen[0]) and torch.equal(plain[1], seen[1])


class _Stop(Exception):
    pass


def test_callback_exception_propagates_and_handle_survives(tiny):
    """an exception at step 3 comes out of the call as itself; the next run on the same pipeline, without a callback, is a fresh run's
    result bit for bit"""
    pipe = _pipe(tiny)

    def stop(i, t, x):
        if i == 3:
            raise _Stop("at 3")
    with pytest.raises(_Stop, match="at 3"):
        _run(tiny, pipe=pipe, eta=0.5, callback=stop)
    after = _run(tiny, pipe=pipe, eta=0.5)
    fresh = _run(tiny, eta=0.5)
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    # eager loop form too
    with pytest.raises(_Stop):
        _run(tiny, pipe=pipe, graph=False, callback=stop)
    assert torch.equal(_run(tiny, pipe=pipe)[1], _run(tiny)[1])


def test_native_abort_code(tiny):
    """a non-zero return of the C callback: LADI_TRYON_CALLBACK_ABORTED, not a generic failure"""
    pipe = _pipe(tiny)
    _run(tiny, pipe=pipe)                     # creates the handle
    lib = _lib.load()
    buf = torch.empty((2, 4, 32, 24), device=U.dev())
    calls = []
    cb = _lib.STEP_CALLBACK(lambda _u, i: calls.append(i) or (7 if i == 1 else 0))
    orig = lib.ladi_tryon_run
    codes = []

    def run(*a):
        assert lib.ladi_tryon_set_step_callback(pipe._tryon, cb, None, 1, ptr(buf)) == 0
        rc = orig(*a)
        codes.append(rc)
        return 0 if rc == _lib.TRYON_CALLBACK_ABORTED else rc
    lib.ladi_tryon_run = run
    try:
        _run(tiny, pipe=pipe)
    finally:
        lib.ladi_tryon_run = orig
        lib.ladi_tryon_set_step_callback(pipe._tryon, _lib.NO_STEP_CALLBACK, None, 1, None)
    assert codes == [_lib.TRYON_CALLBACK_ABORTED] and calls == [0, 1]
    assert "step callback returned 7" in _lib.last_error()
