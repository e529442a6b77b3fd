"""Deep-feature cache (DeepCache on the full-resolution level) on the device: the capturing and the shallow forward of the stand-alone UNet
entry against tests/feature_cache_ref.py, the rows of the cache, then the tiny model end to end (fused hipGraph, fused eager, modular, lanes)
against ref_tryon.tryon_reference, the bit-equalities the feature promises, its combinations, and one case at the released size."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import dtype_code, ptr, stream_ptr
from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import strength_ref as SR
from tests import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, op={})


# ------------------------------------------------------------------------------------------------------------------ operator level
T0, T1 = 481, 461


def _fwd(unet, x, t, mode, branch, sample0=None, expect_error=False):
    """ladi_unet_forward (mode None), ladi_unet_forward_cached (sample0 None) or ladi_unet_forward_cached_rows on the device -> fp32 cpu
    [n, 4, h, w]; expect_error: -> (rc, message) instead"""
    lib = _lib.load()
    xd = x.to(U.dev()).contiguous()
    n, _, h, w = xd.shape
    out = torch.full((n, unet.cfg["out_channels"], h, w), float("nan"), dtype=xd.dtype, device=xd.device)
    a = (unet.h, ptr(xd), dtype_code(xd), n, h, w, float(t), ptr(out), dtype_code(out))
    if mode is None:
        rc = lib.ladi_unet_forward(*a, stream_ptr())
    elif sample0 is None:
        rc = lib.ladi_unet_forward_cached(*a, mode, branch, stream_ptr())
    else:
        rc = lib.ladi_unet_forward_cached_rows(*a, mode, branch, sample0, stream_ptr())
    torch.cuda.synchronize()
    if expect_error:
        return rc, _lib.last_error()
    assert rc == 0, _lib.last_error()
    return out.float().cpu()


def _op_case(tiny, hw, n=2):
    """inputs of the operator tests at one latent size, and the references shared by them: the oracle's whole forward at (x0, T0), the
    capture of every branch there, the reference's shallow forward at (x1, T1) from it"""
    key = (hw, n)
    if key not in tiny["op"]:
        g = torch.Generator().manual_seed(11)
        x0 = torch.randn((n, 31) + hw, generator=g).half().float()
        x1 = (0.7 * x0 + 0.7 * torch.randn((n, 31) + hw, generator=g)).half().float()
        ehs = torch.randn((n, 8, tiny["ucfg"]["cross_attention_dim"]), generator=g).half().float()
        sd, cfg = tiny["sd"]["unet"], tiny["ucfg"]
        c = dict(x0=x0, x1=x1, ehs=ehs, cap={}, shallow={})
        for k in (0, 1, 2):
            c["whole"], c["cap"][k] = RU.unet_forward(sd, cfg, x0, T0, ehs, cache=("capture", k))
            c["shallow"][k] = RU.unet_forward(sd, cfg, x1, T1, ehs, cache=("shallow", k, c["cap"][k]))
        tiny["op"][key] = c
    return tiny["op"][key]


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_capture_changes_nothing(tiny, hw):
    """the capturing forward launches what the plain forward launches plus one copy: bit-equal output, for every branch"""
    c = _op_case(tiny, hw)
    unet = tiny["mod"]["unet"]
    unet.set_context(c["ehs"].to(U.dev()))
    plain = _fwd(unet, c["x0"], T0, None, 0)
    assert torch.isfinite(plain).all()
    for k in (0, 1, 2):
        assert torch.equal(_fwd(unet, c["x0"], T0, 1, k), plain), k
    assert torch.equal(_fwd(unet, c["x0"], T0, 0, 0), plain)          # mode 0 is the plain forward


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_shallow_forward_vs_reference(tiny, hw, k):
    """capture at (x0, t = 481), shallow at (x1 != x0, t = 461) against the reference doing the same from its own cache; thresholds of
    test_unet_forward_tiny (PSNR >= 55 dB, rel-L2 <= 5e-3): a capture + shallow pair runs a subset of one whole forward's layers.  26x19
    (image 208x152) is no multiple of 8: the cached tensor has the size of the skip it is concatenated with."""
    c = _op_case(tiny, hw)
    unet = tiny["mod"]["unet"]
    unet.set_context(c["ehs"].to(U.dev()))
    _fwd(unet, c["x0"], T0, 1, k)
    got = _fwd(unet, c["x1"], T1, 2, k)
    ref = c["shallow"][k]
    ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
    print("shallow forward %dx%d branch %d: PSNR %.2f dB, rel-L2 %.3g" % (hw + (k, ps, rl)))
    U.record_parity("feature_cache_shallow_tiny_%dx%d_k%d" % (hw + (k,)), dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert ps >= 55.0 and rl <= 5e-3, (ps, rl)
    # the shallow forward is another function than the whole forward at (x1, T1): the comparison sees the cache
    assert U.psnr(got, _fwd(unet, c["x1"], T1, None, 0)) < 55.0


@pytest.mark.parametrize("k", [0, 1, 2])
def test_shallow_at_the_captured_input_is_the_whole_forward(tiny, k):
    """shallow at the captured (x0, t) against the GPU's own whole output: at least as close as that output is to the oracle.  Bit equality is
    not promised: the cached half brings no statistics rows, its GroupNorm sums are recomputed in another order (recorded)."""
    c = _op_case(tiny, (32, 24))
    unet = tiny["mod"]["unet"]
    unet.set_context(c["ehs"].to(U.dev()))
    whole = _fwd(unet, c["x0"], T0, 1, k)
    shallow = _fwd(unet, c["x0"], T0, 2, k)
    p_self, p_oracle = U.psnr(shallow, whole), U.psnr(whole, c["whole"])
    bit = torch.equal(shallow, whole)
    print("same input branch %d: PSNR(shallow, whole) %.2f dB, PSNR(whole, oracle) %.2f dB, bit-equal %s" % (k, p_self, p_oracle, bit))
    U.record_parity("feature_cache_same_input_tiny_k%d" % k, dict(psnr_self_db=(None if bit else round(p_self, 2)),
                                                                  psnr_oracle_db=round(p_oracle, 2), bit_equal=bit))
    assert p_oracle >= 55.0
    assert p_self >= p_oracle, (p_self, p_oracle)


def test_cache_rows_and_staleness(tiny):
    """the cache is indexed by sample: a capture over n = 4, then a sub-batch capture of samples [2, 4) with other inputs; a shallow forward
    over n = 4 matches the reference that mixes the two captures row-wise.  A shallow call at another (n, h, w) or branch, or after a
    set_context, is an error with a message."""
    n, hw, k = 4, (32, 24), 1
    g = torch.Generator().manual_seed(23)
    xa, xb, xc = [torch.randn((n, 31) + hw, generator=g).half().float() for _ in range(3)]
    ehs = torch.randn((n, 8, tiny["ucfg"]["cross_attention_dim"]), generator=g).half().float()
    sd, cfg = tiny["sd"]["unet"], tiny["ucfg"]
    _, cap_a = RU.unet_forward(sd, cfg, xa, T0, ehs, cache=("capture", k))
    out_b_ref, cap_b = RU.unet_forward(sd, cfg, xb[2:], 441, ehs[2:], cache=("capture", k))
    ref = RU.unet_forward(sd, cfg, xc, T1, ehs, cache=("shallow", k, torch.cat([cap_a[:2], cap_b])))
    unet = tiny["mod"]["unet"]
    unet.set_context(ehs.to(U.dev()))
    _fwd(unet, xa, T0, 1, k)
    out_b = _fwd(unet, xb[2:], 441, 1, k, sample0=2)
    assert U.psnr(out_b, out_b_ref) >= 55.0                       # the sub-batch forward used rows [2, 4) of the context
    got = _fwd(unet, xc, T1, 2, k)
    ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
    print("mixed rows: PSNR %.2f dB, rel-L2 %.3g" % (ps, rl))
    assert ps >= 55.0 and rl <= 5e-3, (ps, rl)
    stale = RU.unet_forward(sd, cfg, xc, T1, ehs, cache=("shallow", k, cap_a))
    assert U.psnr(got[2:], stale[2:]) < 55.0 and U.psnr(got[:2], stale[:2]) >= 55.0      # rows [2, 4) came from the second capture
    # a sub-batch shallow forward reads its own rows
    sub = _fwd(unet, xc[2:], T1, 2, k, sample0=2)
    assert U.psnr(sub, ref[2:]) >= 55.0
    # misuse: errors with a message
    for what, args in (("another branch", (xc, T1, 2, 0)), ("another size", (xc[:, :, :16, :16], T1, 2, k))):
        rc, msg = _fwd(unet, *args, expect_error=True)
        assert rc != 0 and "without a feature cache captured" in msg, (what, rc, msg)
    rc, msg = _fwd(unet, xc[:2], T1, 2, k, expect_error=True)
    assert rc != 0 and "not the context batch" in msg, (rc, msg)
    rc, msg = _fwd(unet, xc, T1, 2, 3, expect_error=True)
    assert rc != 0 and "branch" in msg
    rc, msg = _fwd(unet, xc, T1, 3, k, expect_error=True)
    assert rc != 0 and "mode" in msg
    assert torch.isfinite(_fwd(unet, xc, T1, 2, k)).all()             # the handle and the cache are fine afterwards
    unet.set_context((ehs * 0.5).to(U.dev()))
    rc, msg = _fwd(unet, xc, T1, 2, k, expect_error=True)
    assert rc != 0 and "since the last ladi_unet_set_context" in msg
    # the shim: a capture over half the context, then a shallow forward over all of it is refused; NativeUNet validates its arguments
    e2 = ehs.to(U.dev())
    unet(xa[:2].to(U.dev()), T0, encoder_hidden_states=e2, feature_cache="capture", cache_branch=k)
    with pytest.raises(_lib.NativeError, match="without a feature cache"):
        unet(xa.to(U.dev()), T0, encoder_hidden_states=e2, feature_cache="reuse", cache_branch=k)
    with pytest.raises(ValueError):
        unet(xa.to(U.dev()), T0, encoder_hidden_states=e2, feature_cache="shallow")
    with pytest.raises(ValueError):
        unet(xa.to(U.dev()), T0, encoder_hidden_states=e2, feature_cache="reuse", cache_branch=3)


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 6
SEED = 77


def _mirror(sched):
    return SR.make_mirror(sched)


def _n_evals(sched, steps=STEPS):
    return steps + 1 if sched == "pndm" else steps


def _tiny_inputs(tiny):
    B, H, W, L_, D = 2, 256, 192, 8, tiny["ucfg"]["cross_attention_dim"]
    inp = P.synthetic_inputs(B, H, W, L=L_, D=D)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp, H, W


def _pipe(tiny, sched):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=_mirror(sched), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, feature_cache, fused=True, graph=True, steps=STEPS, guidance=7.5, **kw):
    """-> (images, latents, shallow evaluations, cond-only evaluations (fused) or None)"""
    inp, H, W = _tiny_inputs(tiny)
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=steps,
               guidance_scale=guidance, output_type="np", fused=fused, use_graph=graph, feature_cache=feature_cache,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu(), pipe.shallow_evals, (pipe.cond_only_evals() if fused else None)


def _ref(tiny, key, sched, interval, branch, steps=STEPS, **kw):
    """ref_tryon.tryon_reference once per case -> (img, latents, counts)"""
    if key not in tiny["ref"]:
        inp, H, W = _tiny_inputs(tiny)
        counts = {}
        img, lat = RT.tryon_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp, steps, sched,
                                      feature_cache=(interval, branch), info=counts, **kw)
        tiny["ref"][key] = (img, lat, counts)
    return tiny["ref"][key]


def _assert_close(what, img, lat, ref_img, ref_lat):
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("%s: image %.2f dB, latents %.2f dB" % (what, p_img, p_lat))
    assert img.shape == ref_img.shape and torch.isfinite(lat).all()
    assert p_lat >= 40.0 and p_img >= 35.0, (what, p_img, p_lat)
    return p_img, p_lat


def _fc(interval, branch):
    return {"interval": interval, "branch": branch}


CASES = [(2, 0), (3, 0), (2, 1), (2, 2)]


def _tiny_run(tiny, sched, interval, branch, arm="graph"):
    """one fused run per (scheduler, case, arm) on a fresh pipeline, shared by the tests below"""
    key = (sched, interval, branch, arm)
    if key not in tiny["run"]:
        tiny["run"][key] = _call(tiny, _pipe(tiny, sched), _fc(interval, branch), fused=arm != "modular", graph=arm == "graph")
    return tiny["run"][key]


@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_off_is_off(tiny, sched):
    """feature_cache = 1 and an all-true sequence are the plain run bit for bit with no shallow evaluation; on ONE pipeline plain, cached,
    plain: the third run equals the first bit for bit (no stale graph, plan or cache), and the cached run is another result"""
    n = _n_evals(sched)
    pipe = _pipe(tiny, sched)
    img_p, lat_p, sh_p, _ = _call(tiny, pipe, None)
    assert sh_p == 0
    img_c, lat_c, sh_c, _ = _call(tiny, pipe, 2)
    assert sh_c == n // 2 and not torch.equal(lat_c, lat_p)
    img_3, lat_3, sh_3, _ = _call(tiny, pipe, None)
    assert sh_3 == 0 and torch.equal(lat_3, lat_p) and torch.equal(img_3, img_p)
    for fc in (1, [True] * n, {"interval": 1, "branch": 2}):
        img_1, lat_1, sh_1, _ = _call(tiny, pipe, fc)
        assert sh_1 == 0 and torch.equal(lat_1, lat_p) and torch.equal(img_1, img_p), fc
    # and the cached run again is the cached run: its graphs are captured anew under their key
    _, lat_c2, sh_c2, _ = _call(tiny, pipe, 2)
    assert sh_c2 == sh_c and torch.equal(lat_c2, lat_c)
    # a fresh pipeline (a fresh native handle) gives the same cached run
    assert torch.equal(_tiny_run(tiny, sched, 2, 0)[1], lat_c)


@pytest.mark.parametrize("interval,branch", CASES)
@pytest.mark.parametrize("sched", ["ddim", "pndm", "dpmpp2m"])
def test_fused_loop_vs_reference_loop(tiny, sched, interval, branch):
    """the fused hipGraph loop against the reference loop with the same plan; thresholds of test_tryon_pipeline_tiny (latents >= 40 dB, image
    >= 35 dB on [0, 1]); the library ran shallow exactly the evaluations of the plan"""
    import ladi_vton_amd as L
    ref_img, ref_lat, counts = _ref(tiny, (sched, interval, branch), sched, interval, branch)
    img, lat, n_sh, n_co = _tiny_run(tiny, sched, interval, branch)
    p_img, p_lat = _assert_close("tiny %s interval %d branch %d" % (sched, interval, branch), img, lat, ref_img, ref_lat)
    U.record_parity("feature_cache_tiny_%s_n%d_k%d" % (sched, interval, branch), dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    flags = L.feature_cache_plan(_n_evals(sched), interval)
    assert n_sh == counts["shallow"] == sum(1 for f in flags if not f) and n_co == 0


@pytest.mark.parametrize("sched,interval,branch", [("pndm", 3, 1), ("ddim", 2, 0)])
def test_graph_equals_eager_bitwise(tiny, sched, interval, branch):
    """replaying the graphs of the forms (whole + capture, shallow) computes what the eager launches compute, bit for bit, as
    test_graph_equals_eager asserts for the plain run"""
    img_g, lat_g, sh_g, _ = _tiny_run(tiny, sched, interval, branch, "graph")
    img_e, lat_e, sh_e, _ = _tiny_run(tiny, sched, interval, branch, "eager")
    assert sh_g == sh_e > 0
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)


def test_fused_and_modular_agree(tiny):
    """the modular path (NativeUNet feature_cache="capture" / "reuse") runs the same plan: image PSNR >= 40 dB against the fused run, the
    threshold of test_fused_and_modular_agree_on_cloth_cond_rate; and it meets the reference like the fused one"""
    ref_img, ref_lat, counts = _ref(tiny, ("ddim", 2, 0), "ddim", 2, 0)
    img_f, _, sh_f, _ = _tiny_run(tiny, "ddim", 2, 0, "graph")
    img_m, lat_m, sh_m, _ = _tiny_run(tiny, "ddim", 2, 0, "modular")
    _assert_close("tiny ddim modular", img_m, lat_m, ref_img, ref_lat)
    assert sh_m == sh_f == counts["shallow"]
    assert U.psnr(img_f, img_m, 1.0) >= 40.0, U.psnr(img_f, img_m, 1.0)


@pytest.mark.parametrize("branch", [0, 2])
def test_lanes_match_single_lane(tiny, branch):
    """two sample-group lanes (each with its own rows of the cache, four graphs' worth of parallel branches) against one lane: latents >= 45
    dB, the threshold of test_unet_lanes_match_single_lane"""
    _, lat_1, sh_1, _ = _tiny_run(tiny, "ddim", 2, branch)
    pipe = _pipe(tiny, "ddim")
    pipe.lanes = 2
    _, lat_2, sh_2, _ = _call(tiny, pipe, _fc(2, branch))
    assert pipe.lib_lanes() == 2 and sh_2 == sh_1
    ref_img, ref_lat, _ = _ref(tiny, ("ddim", 2, branch), "ddim", 2, branch)
    assert U.psnr(lat_2, ref_lat) >= 40.0
    assert U.psnr(lat_2, lat_1) >= 45.0, U.psnr(lat_2, lat_1)


@pytest.mark.parametrize("arm", ["graph", "eager", "modular"])
def test_with_a_guidance_interval_and_a_promotion(tiny, arm):
    """CFG on evaluations 2-4 of 6, whole every third: evaluation 2 would run shallow over 2B samples after the cond-only whole evaluation 0
    and is promoted; 1 and 5 run shallow cond-only.  shallow_evals and cond_only_evals against feature_cache_plan, the run against the reference"""
    import ladi_vton_amd as L
    table = L.guidance_interval(STEPS, 7.5, 0.3, 0.7)
    co = [not g > 1.0 for g in table]
    flags = L.feature_cache_plan(STEPS, 3, co)
    assert flags == [True, False, True, True, False, False]
    ref_img, ref_lat, counts = _ref(tiny, "guided", "ddim", 3, 0, table=table)
    assert counts["flags"] == flags
    img, lat, n_sh, n_co = _call(tiny, _pipe(tiny, "ddim"), 3, fused=arm != "modular", graph=arm == "graph", guidance=table)
    _assert_close("tiny guided + promotion, %s" % arm, img, lat, ref_img, ref_lat)
    assert n_sh == sum(1 for f in flags if not f) == counts["shallow"] == 3
    if arm != "modular":
        assert n_co == sum(co) == counts["cond_only"] == 3


def test_with_a_strength_tail(tiny):
    """strength = 0.5 of 12 steps: the plan indexes the tail's 6 evaluations"""
    inp, H, W = _tiny_inputs(tiny)
    init = SR.synthetic_init(2, H // 8, W // 8)
    ref_img, ref_lat, counts = _ref(tiny, "strength", "ddim", 2, 0, steps=12, init_latents=init, first_step=6)
    assert counts["evals"] == 6 and counts["shallow"] == 3
    img, lat, n_sh, _ = _call(tiny, _pipe(tiny, "ddim"), 2, steps=12, strength=0.5, init_latents=init)
    _assert_close("tiny strength tail", img, lat, ref_img, ref_lat)
    assert n_sh == 3
    # a plan of the whole run's length is refused before anything is launched
    with pytest.raises(ValueError, match="12 entries but the scheduler runs 6"):
        _call(tiny, _pipe(tiny, "ddim"), [1, 0] * 6, steps=12, strength=0.5, init_latents=init)


def test_with_a_step_callback(tiny):
    """a callback with callback_steps = 1 sees every i once and the run equals the run without it bit for bit (the callback points sit
    between graph launches; the cache is not touched by them)"""
    seen = []
    img, lat, n_sh, _ = _call(tiny, _pipe(tiny, "pndm"), _fc(2, 1), callback=lambda i, t, x: seen.append(i), callback_steps=1)
    assert seen == list(range(STEPS + 1)) and n_sh == (STEPS + 1) // 2
    img_0, lat_0, _, _ = _tiny_run(tiny, "pndm", 2, 1)
    assert torch.equal(lat, lat_0) and torch.equal(img, img_0)


def test_with_euler_ancestral_step_noise(tiny):
    """Euler-ancestral: the per-step noise stays indexed per evaluation; a seeded CPU generator on both sides supplies it"""
    ref_img, ref_lat, counts = _ref(tiny, "euler_a", "euler_a", 2, 0, generator=torch.Generator().manual_seed(SEED))
    img, lat, n_sh, _ = _call(tiny, _pipe(tiny, "euler_a"), 2, generator=torch.Generator().manual_seed(SEED))
    _assert_close("tiny euler_a", img, lat, ref_img, ref_lat)
    assert n_sh == counts["shallow"] == 3


def test_misuse_fails_before_anything_is_launched(tiny, lib):
    """the C setters and the run refuse a bad plan with a message, and the handle stays usable"""
    pipe = _pipe(tiny, "pndm")
    inp, H, W = _tiny_inputs(tiny)
    d = U.dev()
    a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
         inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, STEPS, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="6 entries, this run has 7 evaluations"):
        pipe._run_fused(*a, feature_cache=([True, False] * 3, 0))                  # PNDM runs steps + 1 evaluations
    assert "feature-cache plan" in _lib.last_error()
    with pytest.raises(_lib.NativeError, match="must start with a whole evaluation"):
        pipe._run_fused(*a, feature_cache=([False] + [True] * 6, 0))
    with pytest.raises(_lib.NativeError, match="branch"):
        pipe._run_fused(*a, feature_cache=([True, False] * 3 + [True], 3))
    pipe._run_fused(*a, feature_cache=([True, False] * 3 + [True], 2))             # the handle is fine afterwards
    assert pipe.shallow_evals == 3
    h = pipe._tryon
    flags = (ctypes.c_ubyte * 2)(1, 0)
    assert lib.ladi_tryon_set_feature_cache(h, flags, -1, 0) < 0
    assert lib.ladi_tryon_set_feature_cache(h, flags, 2, -1) < 0 and "branch" in _lib.last_error()
    assert lib.ladi_tryon_set_feature_cache(h, None, 0, 0) == 0
    assert lib.ladi_tryon_shallow_evals(None) == -1


# ------------------------------------------------------------------------------------------------------------------ released size
@pytest.fixture(scope="module")
def full():
    import ladi_vton_amd as L
    cfg = C.UNET_FULL
    sd = C.synth_state_dict(C.unet_shapes(cfg), "unet.")
    return dict(cfg=cfg, sd=sd, unet=L.NativeUNet(cfg, sd))


def test_full_unet_capture_and_shallow(full):
    """UNET_FULL, n = 2 at latent 64x48: the product's tile selections for the level-0 shapes with a two-source input whose first half is the
    cache.  Capture changes nothing (bit-equal); shallow at the captured input is at least as close to the GPU's whole output as that is to
    the oracle; shallow at another input and timestep is finite."""
    cfg, sd, unet = full["cfg"], full["sd"], full["unet"]
    g = torch.Generator().manual_seed(5)
    n, h, w = 2, 64, 48
    x0 = torch.randn((n, 31, h, w), generator=g).half().float()
    x1 = (0.7 * x0 + 0.7 * torch.randn((n, 31, h, w), generator=g)).half().float()
    ehs = torch.randn((n, 77, 1024), generator=g).half().float()
    ref = M.unet_forward(sd, cfg, x0, 741, ehs)
    unet.set_context(ehs.to(U.dev()))
    plain = _fwd(unet, x0, 741, None, 0)
    p_oracle = U.psnr(plain, ref)
    assert p_oracle >= 50.0, p_oracle                                   # the threshold of test_full_unet_forward_vs_oracle
    rec = {}
    for k in (0, 1, 2):
        assert torch.equal(_fwd(unet, x0, 741, 1, k), plain), k
        shallow = _fwd(unet, x0, 741, 2, k)
        bit = torch.equal(shallow, plain)
        p_self = U.psnr(shallow, plain)
        print("full branch %d: PSNR(shallow, whole) %.2f dB, PSNR(whole, oracle) %.2f dB, bit-equal %s" % (k, p_self, p_oracle, bit))
        rec[str(k)] = dict(psnr_self_db=(None if bit else round(p_self, 2)), bit_equal=bit)
        assert p_self >= p_oracle, (k, p_self, p_oracle)
        other = _fwd(unet, x1, 721, 2, k)
        assert torch.isfinite(other).all() and not torch.equal(other, shallow)
    rec["psnr_oracle_db"] = round(p_oracle, 2)
    U.record_parity("feature_cache_same_input_full", rec)
