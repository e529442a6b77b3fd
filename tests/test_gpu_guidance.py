"""Guidance schedule, CFG cut-off and guidance rescale on the device: the statistics kernel (ladi_op_cfg_stats) and the guided step kernel
(ladi_op_sched_run_guided) against tests/guidance_ref.py, then the tiny model end to end (fused hipGraph, fused eager, modular) against
ref_tryon.tryon_reference, the bit-equalities the feature promises, and its misuse."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import guidance_ref as G
from tests import ref_tryon as RT
from tests import util as U

pytestmark = pytest.mark.gpu

# one block of the step kernel; 351 pixels: a 256-thread block of the step kernel straddles two samples, hw is odd
SHAPES = [(2, 8, 12), (3, 9, 13)]


# ------------------------------------------------------------------------------------------------------------------ statistics kernel
def _eps_pair(B, hw, seed):
    g = torch.Generator().manual_seed(seed)
    eu = torch.randn((B, hw, 4), generator=g) * 0.8 + 0.05
    ec = torch.randn((B, hw, 4), generator=g) * (torch.arange(B).view(B, 1, 1) * 0.3 + 0.6) - 0.1       # another std per sample
    return torch.cat([eu, ec]).half()


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_cfg_stats_vs_reference(lib, B, h, w, ld):
    """factor[b] = phi * std(c_b) / std(u_b + g (c_b - u_b)) + (1 - phi) against the float64 reference over the same fp16 values: relative
    error <= 1e-5 (the bound of the fp32 scheduler arithmetic against its mirror); two calls are bit-equal; with ld = 8 the lanes 4..7 and the
    rows around the view hold NaN and are never read"""
    hw, gs, phi = h * w, 7.5, 0.7
    eps = _eps_pair(B, hw, 5)
    ge = U.guarded(eps.reshape(2 * B * hw, 4), ld=ld)
    e64 = eps.double()
    ref = G.rescale_factor(G.guided_eps(e64[:B], e64[B:], gs), e64[B:], phi).reshape(B)
    out = torch.full((2, B + 2), -7.0, device=U.dev())
    for k in range(2):
        rc = lib.ladi_op_cfg_stats(ctypes.c_void_p(ge.ptr), ld, B, hw, gs, phi, ptr(out[k]), stream_ptr())
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    rel = ((got[0, :B].double() - ref) / ref).abs().max().item()
    print("cfg_stats B=%d hw=%d ld=%d: max rel err %.3g, factors %s" % (B, hw, ld, rel, got[0, :B].tolist()))
    assert torch.isfinite(got[0, :B]).all() and rel <= 1e-5, rel
    assert torch.equal(got[0], got[1])
    assert (got[:, B:] == -7.0).all()
    U.assert_untouched(ge, "cfg_stats eps")
    # phi = 0 is the identity, phi = 1 the plain ratio
    for p, want in ((0.0, torch.ones(B, dtype=torch.float64)), (1.0, (ref - (1 - phi)) / phi)):
        assert lib.ladi_op_cfg_stats(ctypes.c_void_p(ge.ptr), ld, B, hw, gs, p, ptr(out[0]), stream_ptr()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert ((out[0, :B].cpu().double() - want) / want).abs().max().item() <= 1e-5


def test_cfg_stats_refuses_bad_arguments(lib):
    e = torch.zeros((2 * 2 * 16, 8), dtype=torch.float16, device=U.dev())
    f = torch.zeros(2, device=U.dev())
    assert lib.ladi_op_cfg_stats(ptr(e), 6, 2, 16, 7.5, 0.5, ptr(f), stream_ptr()) < 0 and "ld_eps" in _lib.last_error()
    assert lib.ladi_op_cfg_stats(ptr(e), 2, 2, 16, 7.5, 0.5, ptr(f), stream_ptr()) < 0
    assert lib.ladi_op_cfg_stats(ptr(e), 8, 2, 16, 7.5, 1.5, ptr(f), stream_ptr()) < 0 and "phi" in _lib.last_error()
    assert lib.ladi_op_cfg_stats(None, 8, 2, 16, 7.5, 0.5, ptr(f), stream_ptr()) < 0


# ------------------------------------------------------------------------------------------------------------------ guided step kernel
def _mirror(kind):
    import ladi_vton_amd as L
    return {"ddim": L.DDIMScheduler, "pndm": L.PNDMScheduler, "dpmpp2m": L.DPMSolverMultistepScheduler,
            "euler_a": L.EulerAncestralDiscreteScheduler}[kind]()


def _schedule(name, n):
    if name == "const":
        return [7.5] * n
    if name == "cutoff":
        return [7.5] * 3 + [1.0] * (n - 3)
    # up and down, two cond-only stretches (one of them scales below 1), back to CFG after each
    return ([7.5, 3.0, 1.0, 0.5, 9.0, 1.0, 0.0, 5.0] + [2.0] * n)[:n]


def _sched_case(kind, B, h, w, sched_name, seed=61):
    sch = _mirror(kind)
    steps = 8
    sch.set_timesteps(steps)
    n = len(sch.timesteps)
    table = _schedule(sched_name, n)
    hw = h * w
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((n, 2 * B, hw, 4), generator=g).half()
    for i in range(n):
        if not G.is_cfg(table[i]):
            eps[i, :B] = float("nan")          # a cond-only evaluation never reads its uncond rows
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    noise = torch.stack([torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(17 + i)) for i in range(n)])
    return sch, steps, n, table, eps, lat0, noise


def _run_guided(lib, sch, steps, n, table, eps_dev_ptr, ld, B, hw, phi, lat0, noise):
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = noise.contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    tab = (ctypes.c_float * n)(*table)
    rc = lib.ladi_op_sched_run_guided(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, eps_dev_ptr, ld, n, B, hw, tab, phi, ptr(L_), ptr(N), n,
                                      stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return L_


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("sched_name", ["const", "cutoff", "mixed"])
@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["ddim", "pndm", "dpmpp2m", "euler_a"])
def test_sched_run_guided_vs_reference(lib, kind, B, h, w, sched_name, phi, monkeypatch):
    """the guided step kernel over a random eps sequence vs sched_reference (the mirror's step() with the reference combine): rel-L2 < 1e-5,
    the bound of test_scheduler_ext_device_vs_mirror; the uncond rows of cond-only evaluations hold NaN and the result is finite"""
    import ladi_vton_amd.schedulers as S
    sch, steps, n, table, eps, lat0, noise = _sched_case(kind, B, h, w, sched_name)
    hw = h * w
    # the mirror draws its step noise through _step_noise: hand it the tensors the device gets, in order
    draws = iter(noise)
    monkeypatch.setattr(S, "_step_noise", lambda shape, dtype, generator, device: next(draws).to(dtype))
    e_nchw = eps.view(n, 2 * B, h, w, 4).permute(0, 1, 4, 2, 3)
    ref = G.sched_reference(sch, e_nchw, table, phi, lat0)
    E = eps.to(U.dev())
    L_ = _run_guided(lib, sch, steps, n, table, ptr(E), 4, B, hw, phi, lat0, noise)
    got = L_.cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    err = U.rel_l2(got, ref)
    print("sched_run_guided %s B=%d hw=%d %s phi=%.1f: rel-L2 %.3g" % (kind, B, hw, sched_name, phi, err))
    assert torch.isfinite(got).all()
    assert err < 1e-5, err


@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["ddim", "pndm", "dpmpp2m", "euler_a"])
def test_sched_run_guided_constant_is_the_scalar_run_bitwise(lib, kind, B, h, w):
    """a constant table with phi = 0 is ladi_op_sched_run_noise_eta with the scalar, bit for bit; so is the strided (ld_eps = 8) form, whose
    lanes 4..7 and surrounding rows hold NaN"""
    sch, steps, n, table, eps, lat0, noise = _sched_case(kind, B, h, w, "const")
    hw = h * w
    E = eps.to(U.dev())
    got = _run_guided(lib, sch, steps, n, table, ptr(E), 4, B, hw, 0.0, lat0, noise)
    ge = U.guarded(eps.reshape(n * 2 * B * hw, 4), ld=8)
    got8 = _run_guided(lib, sch, steps, n, table, ctypes.c_void_p(ge.ptr), 8, B, hw, 0.0, lat0, noise)
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = noise.contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    rc = lib.ladi_op_sched_run_noise_eta(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, ptr(E), n, B, hw, 1, 7.5, ptr(L_), ptr(N), n, stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(got, L_) and torch.equal(got8, L_)
    U.assert_untouched(ge, "sched_run_guided eps")


def test_sched_run_guided_strided_rescale_matches_dense(lib):
    """ld_eps = 8 between poisoned lanes with phi > 0 and a mixed table: bit-equal to the dense run (the statistics and the step kernel read
    the same view)"""
    B, h, w = SHAPES[1]
    sch, steps, n, table, eps, lat0, noise = _sched_case("ddim", B, h, w, "mixed")
    E = eps.to(U.dev())
    dense = _run_guided(lib, sch, steps, n, table, ptr(E), 4, B, h * w, 0.7, lat0, noise)
    ge = U.guarded(eps.reshape(n * 2 * B * h * w, 4), ld=8)
    strided = _run_guided(lib, sch, steps, n, table, ctypes.c_void_p(ge.ptr), 8, B, h * w, 0.7, lat0, noise)
    assert torch.isfinite(dense).all() and torch.equal(dense, strided)


def test_sched_run_guided_refuses_bad_tables(lib):
    B, hw, steps = 1, 16, 5
    E = torch.zeros((steps, 2 * B, hw, 4), dtype=torch.float16, device=U.dev())
    L_ = torch.zeros((B, hw, 4), device=U.dev())

    def run(table, phi=0.0, ld=4):
        tab = (ctypes.c_float * len(table))(*table)
        return lib.ladi_op_sched_run_guided(0, steps, None, 0.0, ptr(E), ld, len(table), B, hw, tab, phi, ptr(L_), None, 0, stream_ptr())
    assert run([7.5] * steps) == 0, _lib.last_error()
    assert run([7.5, -1.0, 7.5, 7.5, 7.5]) < 0 and "negative or not finite" in _lib.last_error()
    assert run([7.5, float("nan"), 7.5, 7.5, 7.5]) < 0
    assert run([7.5] * (steps + 1)) < 0 and "evals exceeds" in _lib.last_error()
    assert run([7.5] * steps, phi=1.5) < 0 and "phi" in _lib.last_error()
    assert run([7.5] * steps, ld=6) < 0 and "ld_eps" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={})


STEPS = 8
ARMS = {"graph": (True, True), "eager": (True, False), "modular": (False, False)}


def _n_evals(sched):
    return STEPS + 1 if sched == "pndm" else STEPS


def _case(sched, case):
    """-> (guidance_scale argument, phi).  interval: CFG on the first 60 % of the evaluations; both: CFG on the middle half, so the run starts
    and ends cond-only and returns to CFG in between"""
    import ladi_vton_amd as L
    n = _n_evals(sched)
    return {"interval": (L.guidance_interval(n, 7.5, 0.0, 0.6), 0.0), "rescale": (7.5, 0.7),
            "both": (L.guidance_interval(n, 7.5, 0.25, 0.75), 0.7)}[case]


def _tiny_inputs(tiny):
    B, H, W, L_, D = 2, 256, 192, 8, tiny["ucfg"]["cross_attention_dim"]
    inp = P.synthetic_inputs(B, H, W, L=L_, D=D)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp, H, W


def _tiny_ref(tiny, sched, case):
    if (sched, case) not in tiny["ref"]:
        gs, phi = _case(sched, case)
        table = gs if isinstance(gs, list) else [gs] * _n_evals(sched)
        inp, H, W = _tiny_inputs(tiny)
        counts = {}
        img, lat = RT.tryon_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp, STEPS,
                                      P.make_scheduler(sched), table=table, phi=phi, info=counts)     # the oracle's own scheduler
        tiny["ref"][(sched, case)] = (img, lat, counts)
    return tiny["ref"][(sched, case)]


def _pipe(tiny, sched):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=L.PNDMScheduler() if sched == "pndm" else L.DDIMScheduler(), emasc=tiny["mod"]["emasc"],
                                           emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, gs, phi, fused=True, graph=True):
    """-> (images, latents, cond-only evaluations the library reports (fused) or None)"""
    inp, H, W = _tiny_inputs(tiny)
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=STEPS,
               guidance_scale=gs, guidance_rescale=phi, output_type="np", fused=fused, use_graph=graph,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu(), (pipe.cond_only_evals() if fused else None)


def _tiny_run(tiny, sched, case, arm):
    """one run per (scheduler, case, arm) on a fresh pipeline (a fresh native handle), shared by the tests below"""
    key = (sched, case, arm)
    if key not in tiny["run"]:
        gs, phi = _case(sched, case) if case != "scalar" else (7.5, 0.0)
        tiny["run"][key] = _call(tiny, _pipe(tiny, sched), gs, phi, *ARMS[arm])
    return tiny["run"][key]


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("case", ["interval", "rescale", "both"])
@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_tryon_tiny_guidance_vs_reference(tiny, sched, case, arm):
    """fused hipGraph (two graphs), fused eager and modular against tryon_reference; thresholds of test_tryon_pipeline_tiny (latents >= 40 dB,
    image >= 35 dB on [0, 1]); the library ran cond-only exactly the evaluations the reference did"""
    ref_img, ref_lat, counts = _tiny_ref(tiny, sched, case)
    img, lat, n_cond = _tiny_run(tiny, sched, case, arm)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny %s %s %s: image %.2f dB, latents %.2f dB, cond-only %s of %d" % (sched, case, arm, p_img, p_lat, n_cond, _n_evals(sched)))
    assert img.shape == ref_img.shape
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)
    if arm != "modular":
        assert n_cond == counts["cond_only"] and counts["full"] + counts["cond_only"] == _n_evals(sched)
        assert n_cond == sum(1 for g in (_case(sched, case)[0] if case != "rescale" else []) if not g > 1.0)


@pytest.mark.parametrize("case", ["interval", "rescale", "both"])
@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_tryon_tiny_graph_equals_eager_bitwise(tiny, sched, case):
    """replaying the two graphs computes what the eager launches compute, bit for bit (the statistics reduction has a fixed order)"""
    img_g, lat_g, _ = _tiny_run(tiny, sched, case, "graph")
    img_e, lat_e, _ = _tiny_run(tiny, sched, case, "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)
    # and neither is the plain scalar run: the comparison above sees the feature
    _, lat_s, n_cond = _tiny_run(tiny, sched, "scalar", "graph")
    assert n_cond == 0 and not torch.equal(lat_s, lat_g)


@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_schedule_without_cfg_is_the_run_without_cfg(tiny, sched):
    """an all-<= 1 schedule is guidance_scale = 1.0 bit for bit (B samples, one graph), every evaluation cond-only; phi > 0 on a run with no CFG
    evaluation is accepted and changes nothing"""
    n = _n_evals(sched)
    _, lat_1, c_1 = _call(tiny, _pipe(tiny, sched), 1.0, 0.0)
    _, lat_s, c_s = _call(tiny, _pipe(tiny, sched), ([1.0, 0.5, 0.0] * n)[:n], 0.0)
    _, lat_p, c_p = _call(tiny, _pipe(tiny, sched), 1.0, 0.7)
    assert torch.equal(lat_1, lat_s) and torch.equal(lat_1, lat_p)
    assert c_1 == c_s == c_p == n


@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_constant_list_is_the_scalar_run_and_nothing_stale_survives(tiny, sched):
    """a constant list (and the callable form of it) equals the scalar run bit for bit; a handle that ran a schedule with rescale and then runs
    the scalar with the schedule switched off equals a fresh scalar run bit for bit (no stale graph, table or factor)"""
    n = _n_evals(sched)
    img_s, lat_s, _ = _tiny_run(tiny, sched, "scalar", "graph")
    img_l, lat_l, c_l = _call(tiny, _pipe(tiny, sched), [7.5] * n, 0.0)
    img_f, lat_f, _ = _call(tiny, _pipe(tiny, sched), lambda i, m: 7.5, 0.0)
    assert c_l == 0 and torch.equal(lat_l, lat_s) and torch.equal(img_l, img_s) and torch.equal(lat_f, lat_s)
    pipe = _pipe(tiny, sched)
    gs, phi = _case(sched, "both")
    _, lat_b, c_b = _call(tiny, pipe, gs, phi)
    assert c_b > 0 and torch.equal(lat_b, _tiny_run(tiny, sched, "both", "graph")[1])
    img_2, lat_2, c_2 = _call(tiny, pipe, 7.5, 0.0)
    assert c_2 == 0 and torch.equal(lat_2, lat_s) and torch.equal(img_2, img_s)
    # and back: the schedule's graphs are captured anew under their key
    _, lat_3, _ = _call(tiny, pipe, gs, phi)
    assert torch.equal(lat_3, lat_b)


def test_misuse_fails_before_anything_is_launched(tiny, lib):
    """a schedule whose length is not the evaluation count fails the run (host-side check, ahead of every launch) with a message in
    ladi_last_error, and the handle stays usable; the setters refuse negative / non-finite scales and a phi outside [0, 1]"""
    pipe = _pipe(tiny, "pndm")
    inp, H, W = _tiny_inputs(tiny)
    d = U.dev()
    a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
         inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, STEPS, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="8 entries, this run has 9 evaluations"):
        pipe._run_fused(*a, guidance_table=[7.5] * STEPS)                       # PNDM runs steps + 1 evaluations
    assert "guidance schedule" in _lib.last_error()
    pipe._run_fused(*a, guidance_table=[7.5] * (STEPS + 1))                     # the handle is fine afterwards
    h = pipe._tryon
    bad = (ctypes.c_float * 3)(7.5, -1.0, 2.0)
    assert lib.ladi_tryon_set_guidance_schedule(h, bad, 3) < 0 and "entry 1" in _lib.last_error()
    nan = (ctypes.c_float * 2)(7.5, float("nan"))
    assert lib.ladi_tryon_set_guidance_schedule(h, nan, 2) < 0
    assert lib.ladi_tryon_set_guidance_rescale(h, 1.5) < 0 and "phi" in _lib.last_error()
    assert lib.ladi_tryon_set_guidance_rescale(h, -0.1) < 0
    assert lib.ladi_tryon_set_guidance_rescale(h, float("nan")) < 0
    # a schedule with an entry > 1 needs the negative prompt embeddings, like guidance_scale > 1
    b = list(a)
    b[5] = None
    with pytest.raises(_lib.NativeError, match="negative_prompt_embeds"):
        pipe._run_fused(*b, guidance_table=[1.0] * STEPS + [2.0])
    assert lib.ladi_tryon_set_guidance_schedule(h, None, 0) == 0 and lib.ladi_tryon_set_guidance_rescale(h, 0.0) == 0
