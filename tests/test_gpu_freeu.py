"""FreeU on the device: the one-launch-per-site kernel against tests/freeu_ref.py element by element (strided views in poisoned buffers, in
place and out of place), the native UNet's forward with FreeU against the reference forward, then the tiny model end to end (fused hipGraph,
fused eager, modular, lanes, with the feature cache) against ref_tryon.tryon_reference, and the graph key.  There is no case at the released
width here: building a UNET_FULL and its reference forward costs ten seconds (the operator cases cover C = 256 | 128: several channel chunks)."""
import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import freeu_ref as R
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import util as U

pytestmark = pytest.mark.gpu

FREEU = (0.9, 0.2, 1.4, 1.6)          # diffusers' recommendation for SD 2.1: s1, s2, b1, b2
FREEU_B = (0.9, 0.5, 1.4, 1.6)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


# ------------------------------------------------------------------------------------------------------------------ operator level
def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(lib, gh, C_h, b, gs, C_s, s, gd, n, H, W):
    """ladi_op_freeu on guarded operands (None: that half is off; gd None: in place) -> rc"""
    rc = lib.ladi_op_freeu(gh.ptr if gh else None, gh.ld if gh else 0, C_h, b, gs.ptr if gs else None, gs.ld if gs else 0, C_s, s,
                           (gd or gs).ptr if gs else None, (gd or gs).ld if gs else 0, n, H, W, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _check_skip(got, x, lp, s, what):
    """|got - ref| <= 2^-10 (|x| + |s - 1| |lp|) + 2^-24 per element: one fp16 ulp of the magnitudes that enter the final sum, twice the
    half ulp of the single rounding; the fp32 sums over at most 768 terms stay below 2^-14 of that"""
    ref = x.double() + (s - 1.0) * lp
    lim = 2.0 ** -10 * (x.double().abs() + abs(s - 1.0) * lp.abs()) + 2.0 ** -24
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), what
    worst = float((err / lim).max())
    print("%s: worst err / limit %.3f" % (what, worst))
    assert bool((err <= lim).all()), (what, worst, int((err > lim).sum()))


@pytest.mark.parametrize("chans", [(16, 8), (48, 24), (256, 128)])
@pytest.mark.parametrize("hw", [(1, 2), (2, 2), (3, 2), (5, 3), (8, 6), (32, 24)])
def test_op_vs_reference(lib, hw, chans):
    """both halves of a site on rows with ld > C inside NaN-poisoned buffers, for (b, s) = (1.4, 0.9) and (1.6, 0.2), inputs randn + 3 and
    (second pair) 200 randn; in place and out of place; everything the contract leaves alone keeps its bits; two launches are bit-equal"""
    n, (H, W), (C_h, C_s) = 2, hw, chans
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C_s)
    for (b, s), amp, off in (((1.4, 0.9), 1.0, 3.0), ((1.6, 0.2), 1.0, 3.0), ((1.6, 0.2), 200.0, 0.0)):
        xh = (amp * torch.randn((n, H, W, C_h), generator=g) + off).half()
        xs = (amp * torch.randn((n, H, W, C_s), generator=g) + off).half()
        lp = R.low_pass(xs.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)                    # float64, NHWC
        what = "%dx%d C %d/%d b %.1f s %.1f amp %g" % (H, W, C_h, C_s, b, s, amp)
        # out of place
        gh, gs, gd = U.guarded(xh, ld=C_h + 8), U.guarded(xs, ld=C_s + 16), U.guarded_out(n * H * W, C_s, ld=C_s + 8)
        assert _launch(lib, gh, C_h, b, gs, C_s, s, gd, n, H, W) == 0, _lib.last_error()
        got_h = gh.cpu().reshape(xh.shape)
        assert torch.equal(got_h[..., :C_h // 2], (xh[..., :C_h // 2].float() * b).half()), what
        assert torch.equal(_bits(got_h[..., C_h // 2:]), _bits(xh[..., C_h // 2:])), what
        assert torch.equal(_bits(gs.cpu()), _bits(xs.reshape(-1, C_s))), what               # the source is read only
        got = gd.cpu().reshape(xs.shape)
        _check_skip(got, xs, lp, s, what + " out of place")
        for gx in (gh, gs, gd):
            U.assert_untouched(gx, what)
        # a second launch of the skip half alone (hidden NULL): the same bits
        gd2 = U.guarded_out(n * H * W, C_s, ld=C_s + 8)
        assert _launch(lib, None, 0, b, gs, C_s, s, gd2, n, H, W) == 0, _lib.last_error()
        assert torch.equal(_bits(gd2.cpu()), _bits(gd.cpu())), what
        assert torch.equal(_bits(gh.cpu().reshape(xh.shape)), _bits(got_h))                # and the backbone was not scaled again
        # in place
        gh, gs = U.guarded(xh, ld=C_h + 8), U.guarded(xs, ld=C_s + 16)
        assert _launch(lib, gh, C_h, b, gs, C_s, s, None, n, H, W) == 0, _lib.last_error()
        assert torch.equal(_bits(gs.cpu()), _bits(gd.cpu())), what                          # in place == out of place, bit for bit
        assert torch.equal(_bits(gh.cpu().reshape(xh.shape)), _bits(got_h)), what
        U.assert_untouched(gh, what)
        U.assert_untouched(gs, what)
        # the backbone half alone (skip NULL)
        gh = U.guarded(xh, ld=C_h + 8)
        assert _launch(lib, gh, C_h, b, None, 0, s, None, n, H, W) == 0, _lib.last_error()
        assert torch.equal(_bits(gh.cpu().reshape(xh.shape)), _bits(got_h)), what
        U.assert_untouched(gh, what)


def test_op_refuses_channel_counts_off_the_vector(lib):
    """C_h = 24 (the half-channel boundary is inside a 16-byte vector) and C_s = 12: an error with a message, nothing launched"""
    n, H, W = 2, 3, 2
    xh, xs = torch.ones((n, H, W, 32)).half(), torch.ones((n, H, W, 16)).half()
    gh, gs = U.guarded(xh), U.guarded(xs)
    for C_h, C_s, word in ((24, 16, "C_h = 24"), (32, 12, "C_s = 12")):
        assert _launch(lib, gh, C_h, 1.4, gs, C_s, 0.9, None, n, H, W) != 0
        assert word in _lib.last_error(), _lib.last_error()
    assert lib.ladi_op_freeu(None, 0, 32, 1.4, None, 0, 16, 0.9, None, 0, n, H, W, stream_ptr()) != 0 and "null" in _lib.last_error()
    assert _launch(lib, gh, 32, 1.4, gs, 16, 0.9, None, n, 0, W) != 0
    torch.cuda.synchronize()
    assert torch.equal(gh.cpu().reshape(xh.shape), xh) and torch.equal(gs.cpu().reshape(xs.shape), xs)


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481


@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    yield dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={})
    mods["unet"].disable_freeu()


@pytest.fixture(autouse=True)
def _freeu_off_between_tests(request):
    """the state is sticky in the native UNet the tests of this module share: every test starts and ends with it off"""
    yield
    if "tiny" in request.fixturenames:
        request.getfixturevalue("tiny")["mod"]["unet"].disable_freeu()


def _forward_case(unet, sd, cfg, n, hw, seed, L_=8):
    """plain -> FreeU -> plain on the device, the reference with FreeU on the CPU -> (plain, on, plain again, reference)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 31) + hw, generator=g).half().float()
    ehs = torch.randn((n, L_, cfg["cross_attention_dim"]), generator=g).half().float()
    xd, ed = x.to(U.dev()), ehs.to(U.dev())
    run = lambda: unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    assert unet.freeu is None
    plain = run()
    unet.enable_freeu(*FREEU)
    assert unet.freeu == FREEU
    on = run()
    unet.disable_freeu()
    assert unet.freeu is None
    return plain, on, run(), RU.unet_forward(sd, cfg, x, T0, ehs, freeu=FREEU)


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_forward_vs_reference(tiny, hw):
    """NativeUNet tiny, n = 2, t = 481: sites 4x3 and 8x6 (32x24), 4x3 and 7x5 (26x19, the any-size path).  Thresholds of
    test_unet_forward_tiny (PSNR >= 55 dB, rel-L2 <= 5e-3); the output is another function than the plain forward; disable_freeu() gives
    the bits the forward had before enable_freeu()"""
    plain, on, again, ref = _forward_case(tiny["mod"]["unet"], tiny["sd"]["unet"], tiny["ucfg"], 2, hw, 11)
    ps, rl = U.psnr(on, ref), U.rel_l2(on, ref)
    print("FreeU forward %dx%d: PSNR %.2f dB, rel-L2 %.3g; against the plain forward %.2f dB" % (hw + (ps, rl, U.psnr(on, plain))))
    U.record_parity("freeu_forward_tiny_%dx%d" % hw, dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert on.shape == ref.shape and torch.isfinite(on).all()
    assert ps >= 55.0 and rl <= 5e-3, (ps, rl)
    assert U.psnr(on, plain) < 55.0
    assert torch.equal(again, plain)


def test_setter_misuse(tiny, lib):
    unet = tiny["mod"]["unet"]
    assert lib.ladi_unet_set_freeu(unet.h, 1, 0.9, float("nan"), 1.4, 1.6) == -1 and "finite" in _lib.last_error()
    assert lib.ladi_unet_set_freeu(unet.h, 1, 0.9, 0.2, float("inf"), 1.6) == -1
    assert lib.ladi_unet_set_freeu(unet.h, 0, float("nan"), 0.2, 1.4, 1.6) == 0        # off ignores the values
    with pytest.raises(_lib.NativeError):
        unet.enable_freeu(0.9, 0.2, 1.4, float("nan"))
    assert unet.freeu is None


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 4
H_IMG, W_IMG = 64, 48


def _tiny_inputs(tiny):
    if "inp" not in tiny:
        inp = P.synthetic_inputs(2, H_IMG, W_IMG, L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny["inp"] = inp
    return tiny["inp"]


def _pipe(tiny):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=L.DDIMScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, freeu, fused=True, graph=True, feature_cache=None):
    """one run with FreeU set through the pipeline -> (images, latents)"""
    inp, d = _tiny_inputs(tiny), U.dev()
    if freeu is None:
        pipe.disable_freeu()
    else:
        pipe.enable_freeu(*freeu)
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H_IMG, width=W_IMG, num_inference_steps=STEPS,
               guidance_scale=7.5, output_type="np", fused=fused, use_graph=graph, feature_cache=feature_cache,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _ref(tiny, freeu, interval=None):
    """ref_tryon.tryon_reference once per case -> (img, latents, counts)"""
    key = (freeu, interval)
    if key not in tiny["ref"]:
        counts = {}
        img, lat = RT.tryon_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], _tiny_inputs(tiny),
                                      STEPS, "ddim", freeu=freeu, feature_cache=(interval, 0), info=counts)
        tiny["ref"][key] = (img, lat, counts)
    return tiny["ref"][key]


def _run(tiny, arm):
    """one FreeU run per arm on a fresh pipeline, shared by the tests below"""
    if arm not in tiny["run"]:
        tiny["run"][arm] = _call(tiny, _pipe(tiny), FREEU, fused=arm != "modular", graph=arm == "graph")
    return tiny["run"][arm]


def _assert_close(what, img, lat, ref_img, ref_lat):
    """thresholds of test_gpu_feature_cache.py's loop test (test_tryon_pipeline_tiny): latents >= 40 dB, image >= 35 dB on [0, 1]"""
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("%s: image %.2f dB, latents %.2f dB" % (what, p_img, p_lat))
    assert img.shape == ref_img.shape and torch.isfinite(lat).all()
    assert p_lat >= 40.0 and p_img >= 35.0, (what, p_img, p_lat)
    return p_img, p_lat


def test_fused_loop_vs_reference_loop(tiny):
    ref_img, ref_lat, _ = _ref(tiny, FREEU)
    img, lat = _run(tiny, "graph")
    p_img, p_lat = _assert_close("tiny FreeU fused graph", img, lat, ref_img, ref_lat)
    U.record_parity("freeu_tiny_ddim", dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    assert U.psnr(lat, _ref(tiny, None)[1]) < 40.0            # and it is not the plain loop


def test_graph_equals_eager_bitwise(tiny):
    img_g, lat_g = _run(tiny, "graph")
    img_e, lat_e = _run(tiny, "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)


def test_fused_and_modular_agree(tiny):
    ref_img, ref_lat, _ = _ref(tiny, FREEU)
    img_f, _ = _run(tiny, "graph")
    img_m, lat_m = _run(tiny, "modular")
    _assert_close("tiny FreeU modular", img_m, lat_m, ref_img, ref_lat)
    assert U.psnr(img_f, img_m, 1.0) >= 40.0, U.psnr(img_f, img_m, 1.0)


def test_no_stale_graph(tiny):
    """one pipeline with use_graph: plain -> FreeU (s2 = 0.2) -> FreeU (s2 = 0.5) -> plain.  The graph key holds the state and the four
    values: runs 1 and 4 are bit-equal, 2 and 3 each meet their own reference and are further apart than the threshold"""
    pipe = _pipe(tiny)
    img_1, lat_1 = _call(tiny, pipe, None)
    img_2, lat_2 = _call(tiny, pipe, FREEU)
    img_3, lat_3 = _call(tiny, pipe, FREEU_B)
    img_4, lat_4 = _call(tiny, pipe, None)
    assert torch.equal(lat_4, lat_1) and torch.equal(img_4, img_1)
    _assert_close("plain", img_1, lat_1, *_ref(tiny, None)[:2])
    _assert_close("FreeU s2 = 0.2", img_2, lat_2, *_ref(tiny, FREEU)[:2])
    _assert_close("FreeU s2 = 0.5", img_3, lat_3, *_ref(tiny, FREEU_B)[:2])
    p = U.psnr(lat_3, lat_2)
    print("s2 = 0.5 against s2 = 0.2: latents %.2f dB" % p)
    assert p < 40.0, p
    assert torch.equal(lat_2, _run(tiny, "graph")[1])           # a fresh pipeline gives the same FreeU run


def test_with_the_feature_cache(tiny):
    """feature_cache = 2: whole evaluations 0 and 2 apply FreeU and refresh the cache, shallow evaluations 1 and 3 have no FreeU site"""
    ref_img, ref_lat, counts = _ref(tiny, FREEU, 2)
    pipe = _pipe(tiny)
    img, lat = _call(tiny, pipe, FREEU, feature_cache=2)
    _assert_close("tiny FreeU + feature cache", img, lat, ref_img, ref_lat)
    assert pipe.shallow_evals == counts["shallow"] == 2


def test_lanes_match_single_lane(tiny):
    """two sample-group lanes against one: latents >= 45 dB, the threshold of test_unet_lanes_match_single_lane"""
    _, lat_1 = _run(tiny, "graph")
    pipe = _pipe(tiny)
    pipe.lanes = 2
    _, lat_2 = _call(tiny, pipe, FREEU)
    assert pipe.lib_lanes() == 2
    assert U.psnr(lat_2, _ref(tiny, FREEU)[1]) >= 40.0
    assert U.psnr(lat_2, lat_1) >= 45.0, U.psnr(lat_2, lat_1)
