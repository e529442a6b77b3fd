"""Starting the fused loop from an image or latents (`strength`) on the device: the start-latents kernel (ladi_op_init_latents) against
tests/strength_ref.py, then the tiny model end to end (fused hipGraph, fused eager, modular) against ref_tryon.tryon_reference for all six
schedulers, the tail identity that pins the mechanism (a run resumed from the latents after evaluation k - 1 reproduces the whole run bit for
bit), the two-pass recipe, stale state, and the interplay with the per-evaluation interfaces."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import ref_tryon as RT
from tests import strength_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

# (B, h, w): one block; 351 pixels: hw is odd and a 256-thread block straddles two samples
SHAPES = [(2, 8, 12), (3, 9, 13)]
# source sizes: the target's own (None), exact 2x up of (8, 12), non-integer up, down, a single sample, exact 2x down of (9, 13)
SOURCES = [None, (4, 6), (5, 7), (16, 24), (1, 1), (18, 26)]


# ------------------------------------------------------------------------------------------------------------------ start-latents kernel
def _planes(t):
    """an NCHW fp32 input between NaN rows: reading outside it turns the result non-finite"""
    return U.guarded(t.reshape(-1, t.shape[-1]).contiguous(), any_ld=True)


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_init_latents_vs_reference(lib, B, h, w, src):
    """k_x * resample(init) + k_n * noise in the loop's pixel-major layout against the float64 start_latents: rel-L2 < 1e-5, the bound
    test_sched_run_guided_vs_reference uses for the fp32 scheduler arithmetic; the output's surroundings stay untouched, two calls are bit-equal"""
    hs, ws = src or (h, w)
    g = torch.Generator().manual_seed(31 * h + hs)
    init, noise = torch.randn((B, 4, hs, ws), generator=g) * 0.9 + 0.1, torch.randn((B, 4, h, w), generator=g)
    k_x, k_n = 0.68075, 0.73251
    ref = R.start_latents(init, noise, k_x, k_n, h, w)
    gi, gn = _planes(init), _planes(noise)
    outs = []
    for _ in range(2):
        go = U.guarded_out(B * h * w, 4, dtype=torch.float32)
        rc = lib.ladi_op_init_latents(ctypes.c_void_p(gi.ptr), hs, ws, ctypes.c_void_p(gn.ptr), B, h, w, k_x, k_n, ctypes.c_void_p(go.ptr), stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        U.assert_untouched(go, "init_latents out")
        outs.append(go.cpu())
    got = outs[0].view(B, h, w, 4).permute(0, 3, 1, 2)
    err = U.rel_l2(got, ref)
    print("init_latents B=%d (%d, %d) -> (%d, %d): rel-L2 %.3g" % (B, hs, ws, h, w, err))
    assert torch.isfinite(got).all() and err < 1e-5, err
    assert torch.equal(outs[0], outs[1])
    U.assert_untouched(gi, "init_latents init")
    U.assert_untouched(gn, "init_latents noise")


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_init_latents_same_size_is_a_layout_change_bitwise(lib, B, h, w):
    """k_x = 1, k_n = 0, NULL noise: NCHW -> pixel-major and nothing else"""
    init = torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(h))
    init[0, 0, 0, 0], init[0, 1, 0, 1] = -0.0, 1e-42         # a negative zero and a subnormal survive
    gi = _planes(init)
    go = U.guarded_out(B * h * w, 4, dtype=torch.float32)
    rc = lib.ladi_op_init_latents(ctypes.c_void_p(gi.ptr), h, w, None, B, h, w, 1.0, 0.0, ctypes.c_void_p(go.ptr), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    want = init.permute(0, 2, 3, 1).reshape(B * h * w, 4).contiguous()
    assert torch.equal(go.cpu().view(torch.int32), want.view(torch.int32))
    U.assert_untouched(go, "init_latents out")


def test_init_latents_refuses_bad_arguments(lib):
    d = U.dev()
    init, noise, out = torch.zeros((1, 4, 4, 4), device=d), torch.zeros((1, 4, 4, 4), device=d), torch.full((16, 4), 3.0, device=d)

    def run(i=init, hs=4, ws=4, n=noise, B=1, h=4, w=4, k_n=0.5, o=out):
        return lib.ladi_op_init_latents(ptr(i), hs, ws, ptr(n), B, h, w, 0.5, k_n, ptr(o), stream_ptr())
    assert run() == 0, _lib.last_error()
    assert run(i=None) < 0 and "null init" in _lib.last_error()
    assert run(o=None) < 0
    for kw in (dict(hs=0), dict(ws=0), dict(B=0), dict(h=0), dict(w=-1)):
        assert run(**kw) < 0 and "size" in _lib.last_error(), kw
    assert run(n=None) < 0 and "null noise" in _lib.last_error()
    assert run(n=None, k_n=0.0) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert (out == 0).all()


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, inp={})


STEPS, STRENGTH, FIRST = 8, 0.5, 4
B_, H_, W_ = 2, 256, 192
ARMS = {"graph": (True, True), "eager": (True, False), "modular": (False, False)}
NOISE_SEED = 5          # the step noise of Euler / Euler-ancestral: one generator, seeded alike for the library and the reference


def _inputs(tiny, H=H_, W=W_):
    if (H, W) not in tiny["inp"]:
        inp = P.synthetic_inputs(B_, H, W, L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny["inp"][(H, W)] = inp
    return tiny["inp"][(H, W)]


def _init(tiny):
    """the synthetic init at the run's own latent size"""
    return R.synthetic_init(B_, H_ // 8, W_ // 8)


def _pipe(tiny, sched):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=R.make_mirror(sched), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, fused=True, graph=True, H=H_, W=W_, **kw):
    """-> (images, latents)"""
    inp = _inputs(tiny, H, W)
    d = U.dev()
    kw.setdefault("generator", torch.Generator().manual_seed(NOISE_SEED))
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=STEPS,
               output_type="np", fused=fused, use_graph=graph, noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _ref(tiny, sched, init=None, first_step=FIRST, key=None, **kw):
    key = (sched, key or "synthetic")
    if key not in tiny["ref"]:
        sd = tiny["sd"]
        tiny["ref"][key] = RT.tryon_reference(sd["unet"], tiny["ucfg"], sd["vae"], tiny["vcfg"], sd["emasc"], _inputs(tiny), STEPS, sched,
                                              init_latents=_init(tiny) if init is None else init, first_step=first_step,
                                              generator=torch.Generator().manual_seed(NOISE_SEED), **kw)
    return tiny["ref"][key]


def _run(tiny, sched, arm):
    """one strength run per (scheduler, arm) on a fresh pipeline (a fresh native handle), shared by the tests below"""
    if (sched, arm) not in tiny["run"]:
        kw = {} if arm == "plain" else dict(strength=STRENGTH, init_latents=_init(tiny))
        tiny["run"][(sched, arm)] = _call(tiny, _pipe(tiny, sched), *ARMS["graph" if arm == "plain" else arm], **kw)
    return tiny["run"][(sched, arm)]


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("sched", R.SCHEDULERS)
def test_tryon_tiny_strength_vs_reference(tiny, sched, arm):
    """B = 2, 256x192, 8 steps, strength 0.5 from synthetic init latents: fused hipGraph, fused eager and modular against tryon_reference;
    the project's tiny thresholds (latents >= 40 dB, image >= 35 dB on [0, 1])"""
    ref_img, ref_lat = _ref(tiny, sched)
    img, lat = _run(tiny, sched, arm)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny strength %s %s: image %.2f dB, latents %.2f dB" % (sched, arm, p_img, p_lat))
    assert img.shape == ref_img.shape and torch.isfinite(lat).all()
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


@pytest.mark.parametrize("sched", R.SCHEDULERS)
def test_tryon_tiny_strength_graph_equals_eager_bitwise(tiny, sched):
    img_g, lat_g = _run(tiny, sched, "graph")
    img_e, lat_e = _run(tiny, sched, "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)
    # and it is not the plain run from noise: the comparisons see the feature
    _, lat_p = _run(tiny, sched, "plain")
    assert not torch.equal(lat_p, lat_g)


def test_strength_one_with_an_init_is_the_plain_run_bitwise(tiny):
    img_p, lat_p = _run(tiny, "ddim", "plain")
    img, lat = _call(tiny, _pipe(tiny, "ddim"), strength=1.0, init_latents=_init(tiny))
    assert torch.equal(lat, lat_p) and torch.equal(img, img_p)


# ------------------------------------------------------------------------------------------------------------------ tail identity
def _fused_args(tiny):
    inp = _inputs(tiny)
    d = U.dev()
    return (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
            inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H_, W_, STEPS, 7.5, 1.0, False, True)


@pytest.fixture(scope="module")
def whole(tiny):
    """the whole 8-step runs with every evaluation's latents traced: scheduler -> (images, latents, trace latents [8, B, 4, h, w], step noise)"""
    out = {}
    for sched in ("ddim", "euler", "euler_a"):
        pipe = _pipe(tiny, sched)
        pipe.trace_evals = STEPS
        noise = None
        if sched == "euler_a":
            g = torch.Generator().manual_seed(23)
            noise = torch.randn((STEPS, B_, 4, H_ // 8, W_ // 8), generator=g)
            img = torch.from_numpy(pipe._run_fused(*_fused_args(tiny), step_noise=noise))
            lat = pipe.last_latents.float().cpu()
        else:
            img, lat = _call(tiny, pipe, cloth_cond_rate=1.0)
        out[sched] = (img, lat, pipe.last_trace["latents"].clone(), noise)
    return out


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("sched", ["ddim", "euler", "euler_a"])
def test_tail_from_traced_latents_reproduces_the_whole_run_bitwise(tiny, whole, sched, k):
    """the latents after evaluation k - 1 of the whole run, handed back as a noisy init at first_step = k, give the whole run's final latents
    and images bit for bit: the tail's tables, time embeddings, first UNet input and step noise are exactly the whole run's from k on"""
    img_w, lat_w, trace, noise = whole[sched]
    pipe = _pipe(tiny, sched)
    if sched == "euler_a":
        img = torch.from_numpy(pipe._run_fused(*_fused_args(tiny), step_noise=noise[k:], init_latents=trace[k - 1], first_step=k, init_is_noisy=True))
        lat = pipe.last_latents.float().cpu()
    else:
        strength = (STEPS - k) / STEPS
        assert R.first_step_of(strength, STEPS) == k
        img, lat = _call(tiny, pipe, strength=strength, init_latents=trace[k - 1], init_is_noisy=True, cloth_cond_rate=1.0)
    assert torch.equal(lat, lat_w), "latents differ (max abs %.3g)" % float((lat - lat_w).abs().max())
    assert torch.equal(img, img_w)


# ------------------------------------------------------------------------------------------------------------------ two-pass recipe
def test_two_pass_low_resolution_latents_as_init(tiny):
    """the README recipe: a 128x96 run's last_latents as init_latents of a 256x192 run at strength 0.5, against the reference handed the same
    low-resolution latents (the resample is then the restated one)"""
    pipe = _pipe(tiny, "ddim")
    _call(tiny, pipe, H=128, W=96)
    low = pipe.last_latents.clone()
    assert tuple(low.shape) == (B_, 4, 16, 12)
    img, lat = _call(tiny, pipe, strength=STRENGTH, init_latents=low)
    ref_img, ref_lat = _ref(tiny, "ddim", init=low.float().cpu(), key="two-pass")
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny two-pass: image %.2f dB, latents %.2f dB" % (p_img, p_lat))
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)
    # the modular path resamples with torch's F.interpolate: the same run within the same thresholds
    img_m, lat_m = _call(tiny, _pipe(tiny, "ddim"), False, False, strength=STRENGTH, init_latents=low)
    assert U.psnr(lat_m, ref_lat) >= 40.0 and U.psnr(img_m, ref_img, peak=1.0) >= 35.0


def test_init_image_is_the_mode_of_its_encode(tiny):
    """init_image of another size than the run's == init_latents = scaling_factor * mode of vae.encode(init_image), bit for bit"""
    image = _inputs(tiny, 128, 96)["image"].to(U.dev())
    pipe = _pipe(tiny, "ddim")
    img_a, lat_a = _call(tiny, pipe, strength=STRENGTH, init_image=image)
    mode = tiny["mod"]["vae"].encode(image)[0].latent_dist.mode()
    init = (tiny["vcfg"]["scaling_factor"] * mode.float()).contiguous()
    assert tuple(init.shape) == (B_, 4, 16, 12)
    img_b, lat_b = _call(tiny, pipe, strength=STRENGTH, init_latents=init)
    assert torch.equal(lat_a, lat_b) and torch.equal(img_a, img_b)
    assert not torch.equal(lat_a, _run(tiny, "ddim", "graph")[1])


# ------------------------------------------------------------------------------------------------------------------ stale state
@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_nothing_stale_survives_an_init(tiny, sched):
    """a handle that ran with an init and then runs without one equals a fresh handle's plain run bit for bit, and the other way round"""
    img_s, lat_s = _run(tiny, sched, "graph")
    img_p, lat_p = _run(tiny, sched, "plain")
    pipe = _pipe(tiny, sched)
    _, lat_1 = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny))
    img_2, lat_2 = _call(tiny, pipe)
    img_3, lat_3 = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny))
    assert torch.equal(lat_1, lat_s)
    assert torch.equal(lat_2, lat_p) and torch.equal(img_2, img_p)
    assert torch.equal(lat_3, lat_s) and torch.equal(img_3, img_s)


# ------------------------------------------------------------------------------------------------------------------ interplay
def test_guidance_schedule_has_the_tails_length(tiny):
    import ladi_vton_amd as L
    table = L.guidance_interval(STEPS - FIRST, 7.5, 0.0, 0.5)          # CFG on the tail's first half, cond-only after
    pipe = _pipe(tiny, "ddim")
    img, lat = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny), guidance_scale=table)
    assert pipe.cond_only_evals() == 2
    ref_img, ref_lat = _ref(tiny, "ddim", key="schedule", table=table)
    assert U.psnr(lat, ref_lat) >= 40.0 and U.psnr(img, ref_img, peak=1.0) >= 35.0
    # a schedule of the whole run's length: refused by the pipeline, and by the library before anything is launched
    with pytest.raises(ValueError, match="8 entries but the scheduler runs 4 evaluations"):
        _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny), guidance_scale=[7.5] * STEPS)
    with pytest.raises(_lib.NativeError, match="8 entries, this run has 4 evaluations"):
        pipe._run_fused(*_fused_args(tiny), guidance_table=[7.5] * STEPS, init_latents=_init(tiny), first_step=FIRST)
    assert "starts at step 4 of 8" in _lib.last_error()
    _, lat_2 = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny), guidance_scale=table)      # the handle is fine afterwards
    assert torch.equal(lat_2, lat)


def test_callback_sees_the_tails_indices_and_timesteps(tiny):
    seen = []
    pipe = _pipe(tiny, "ddim")
    _, lat = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny), callback=lambda i, t, x: seen.append((i, int(t), tuple(x.shape))))
    whole_ts = R.make_mirror("ddim")
    whole_ts.set_timesteps(STEPS)
    want = whole_ts.timesteps.tolist()[FIRST:]
    assert seen == [(i, t, (B_, 4, H_ // 8, W_ // 8)) for i, t in enumerate(want)]
    assert pipe.scheduler.timesteps.tolist() == want
    assert torch.equal(lat, _run(tiny, "ddim", "graph")[1])            # an untouched round trip changes no bit


def test_out_of_range_starts_are_refused_with_a_message(tiny, lib):
    """a PNDM tail of one step, through the pipeline and at the library (before anything is launched; the handle stays usable); the setter's
    own refusals"""
    pipe = _pipe(tiny, "pndm")
    with pytest.raises(ValueError, match="PNDM tail needs at least 2 steps"):
        _call(tiny, pipe, strength=1.0 / STEPS, init_latents=_init(tiny))
    with pytest.raises(_lib.NativeError, match="PNDM tail needs at least 2 steps"):
        pipe._run_fused(*_fused_args(tiny), init_latents=_init(tiny), first_step=STEPS - 1)
    with pytest.raises(_lib.NativeError, match="first_step 8 out of range"):
        pipe._run_fused(*_fused_args(tiny), init_latents=_init(tiny), first_step=STEPS)
    _, lat = _call(tiny, pipe, strength=STRENGTH, init_latents=_init(tiny))
    assert torch.equal(lat, _run(tiny, "pndm", "graph")[1])
    h = pipe._tryon
    x = _init(tiny).to(U.dev())
    assert lib.ladi_tryon_set_init(h, ptr(x), 0, 24, 4, 0) < 0 and "size" in _lib.last_error()
    assert lib.ladi_tryon_set_init(h, ptr(x), 32, -1, 4, 0) < 0
    assert lib.ladi_tryon_set_init(h, ptr(x), 32, 24, -1, 0) < 0 and "negative" in _lib.last_error()
    assert lib.ladi_tryon_set_init(None, ptr(x), 32, 24, 4, 0) < 0
    assert lib.ladi_tryon_set_init(h, None, 0, 0, 0, 0) == 0
    # Euler-ancestral: step noise counted in the tail's evaluations
    pe = _pipe(tiny, "euler_a")
    noise = torch.randn((STEPS - FIRST - 1, B_, 4, H_ // 8, W_ // 8), generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="step noise"):
        pe._run_fused(*_fused_args(tiny), step_noise=noise, init_latents=_init(tiny), first_step=FIRST)
