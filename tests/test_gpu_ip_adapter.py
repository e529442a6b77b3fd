"""The IP-Adapter image prompt on the device: the image-term kernel on strided views in poisoned buffers against the float64 references and
bounds of tests/ip_adapter_cases.py, the native UNet's forward with an image context against tests/ip_adapter_ref.py, then the tiny model
end to end (fused hipGraph, fused eager, modular, lanes, with the other sampler switches), the graph key and the misuse."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import stream_ptr
from tests import ip_adapter_cases as IC
from tests import ip_adapter_ref as R
from tests import pag_ref as PG
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import tiny_tryon as TT
from tests import util as U

pytestmark = pytest.mark.gpu
N_TOK, E = 4, 64


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ the operator
def _place(case, pad):
    n, T, Cc = case["q"].shape
    gq = U.guarded(case["q"].reshape(n * T, Cc), ld=Cc + pad)
    gk = U.guarded(case["kv"].reshape(-1, 2 * Cc), ld=2 * Cc + pad)
    go = U.guarded(case["o"].reshape(n * T, Cc), ld=Cc + pad)
    return gq, gk, go


def _launch(lib, gq, gk, go, n, T, heads, N, scale):
    Cc = heads * 64
    return lib.ladi_op_ip_attn_add(ctypes.c_void_p(gq.ptr), gq.ld, T * gq.ld, ctypes.c_void_p(gk.ptr), gk.ld, N * gk.ld, ctypes.c_void_p(gk.col(Cc)),
                                   gk.ld, N * gk.ld, ctypes.c_void_p(go.ptr), go.ld, T * go.ld, n, heads, T, N, scale, stream_ptr())


@pytest.mark.parametrize("c", IC.CASES, ids=IC.case_id)
def test_ip_attn_add_op(lib, c):
    """o += scale softmax(q k^T / 8) v in place: every element within ulp16(ref) + the derived bound, nothing outside the views changes, q and
    k | v are read only, two launches from the same input are bit-equal"""
    n, T, heads, N, pad, scale, kind = c
    case = IC.make_case(*c)
    outs = []
    for _ in range(2):
        gq, gk, go = _place(case, pad)
        rc = _launch(lib, gq, gk, go, n, T, heads, N, scale)
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        outs.append(go.cpu())
        for g, what in ((gq, "q"), (gk, "k | v"), (go, "o")):
            U.assert_untouched(g, "ip_attn_add " + what)
        assert torch.equal(_bits(gq.cpu()), _bits(case["q"].reshape(n * T, -1))) and torch.equal(_bits(gk.cpu()), _bits(case["kv"].reshape(n * N, -1)))
    ratio = U.check_elem(outs[0].reshape(n, T, -1), case["ref"], case["bound"], "ip_attn_add " + IC.case_id(c))
    print("ip_attn_add %s: worst error over bound %.3f" % (IC.case_id(c), ratio))
    U.record_parity("ip_attn_add_" + IC.case_id(c), dict(err_over_bound=round(ratio, 4)))
    assert ratio <= 1.0
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_ip_attn_add_refusals(lib):
    """N = 0, N = 65, misaligned strides and bases: -1 with a message, nothing written"""
    c = (3, 5, 5, 4, 8, 0.6, "plain")
    n, T, heads, N = c[:4]
    gq, gk, go = _place(IC.make_case(*c), 8)
    before = _bits(go.buf.cpu())
    Cc = heads * 64

    def run(N_=N, ldq=gq.ld, ldk=gk.ld, ldo=go.ld, q=gq.ptr, o=go.ptr, so=T * go.ld):
        return lib.ladi_op_ip_attn_add(ctypes.c_void_p(q) if q else None, ldq, T * ldq, ctypes.c_void_p(gk.ptr), ldk, N * ldk,
                                       ctypes.c_void_p(gk.col(Cc)), ldk, N * ldk, ctypes.c_void_p(o) if o else None, ldo, so, n, heads, T, N_, 0.6,
                                       stream_ptr())
    assert run(N_=0) == -1 and "N = 0" in _lib.last_error()
    assert run(N_=65) == -1 and "N = 65" in _lib.last_error()
    assert run(ldq=Cc + 4) == -1 and run(ldk=2 * Cc + 4) == -1 and run(ldo=Cc + 4) == -1
    assert run(ldo=Cc - 8) == -1 and run(so=T * go.ld + 4) == -1
    assert run(q=gq.ptr + 2) == -1 and run(o=go.ptr + 2) == -1 and "aligned" in _lib.last_error()
    assert run(q=None) == -1 and run(o=None) == -1
    torch.cuda.synchronize()
    assert torch.equal(_bits(go.buf.cpu()), before)


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481
ONES = [1.0] * 16
MID2 = [0.0] * 6 + [2.0] + [0.0] * 9


@pytest.fixture(scope="module")
def tiny():
    t = TT.build()
    sd_ip = R.make_adapter(t["ucfg"], N_TOK, E)
    assert t["mod"]["unet"].ip_adapter_info is None
    t["mod"]["unet"].load_ip_adapter(R.to_diffusers(sd_ip, 2, numbered=True))       # diffusers' nested layout with numbered keys
    g = torch.Generator().manual_seed(77)
    emb = torch.randn((2, E), generator=g).half().float()
    neg = (torch.randn((2, E), generator=g) * 0.5).half().float()
    t.update(ip=sd_ip, emb=emb, neg=neg)
    yield t


@pytest.fixture(autouse=True)
def _defaults_between_tests(request):
    """scales, PAG layers and FreeU are sticky in the native UNet the tests of this module share"""
    yield
    if "tiny" in request.fixturenames:
        u = request.getfixturevalue("tiny")["mod"]["unet"]
        u.set_pag_applied_layers("mid")
        u.disable_freeu()
        if u.ip_adapter_info is not None:
            u.set_ip_adapter_scale(1.0)


def _fwd_inputs(tiny, hw):
    """n = 4: samples 2, 3 are copies of samples 0, 1 (inputs and context), with their own image embeddings"""
    if ("ip",) + hw not in tiny["fwd"]:
        emb4 = torch.cat([tiny["emb"], tiny["neg"]])
        tiny["fwd"][("ip",) + hw] = (emb4, emb4.to(U.dev()))
    return TT.unet_inputs(tiny, hw) + tiny["fwd"][("ip",) + hw]


def _close(what, got, ref, key=None):
    ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
    print("%s: PSNR %.2f dB, rel-L2 %.3g" % (what, ps, rl))
    if key:
        U.record_parity(key, dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert ps >= 55.0 and rl <= 5e-3, (what, ps, rl)


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_forward_vs_reference(tiny, hw):
    """NativeUNet tiny, n = 4, t = 481, thresholds of test_unet_forward_tiny (PSNR >= 55 dB, rel-L2 <= 5e-3) against ref_unet.unet_forward:
    every block at scale 1, the mid block alone at scale 2; both are another function than the plain forward; scale 0, no image context and
    a cleared context are the plain forward bit for bit"""
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed, emb, embd = _fwd_inputs(tiny, hw)
    run = lambda **kw: unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu()
    plain = run()
    assert unet.ip_adapter_info == (N_TOK, E) and unet.ip_adapter_scale == ONES
    on = run(ip_image_embeds=embd)
    tok = R.image_proj(tiny["ip"], emb)
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, ip=(tiny["ip"], tok, ONES))
    _close("IP forward %dx%d" % hw, on, ref, "ip_forward_tiny_%dx%d" % hw)
    pp = U.psnr(on, plain)
    print("IP forward %dx%d against plain: %.2f dB" % (hw + (pp,)))
    assert pp < 55.0, pp
    assert torch.equal(run(ip_image_embeds=embd[:, None]), on)                     # [n, 1, E]
    unet.set_ip_adapter_scale({"mid": 2.0})
    assert unet.ip_adapter_scale == MID2
    mid = run(ip_image_embeds=embd)
    _close("IP forward %dx%d, mid block alone" % hw, mid, RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, ip=(tiny["ip"], tok, MID2)),
           "ip_forward_tiny_mid_%dx%d" % hw)
    pm = U.psnr(mid, plain)
    assert pm < 55.0 and not torch.equal(mid, on), pm
    unet.set_ip_adapter_scale(0.0)
    assert torch.equal(run(ip_image_embeds=embd), plain)                           # every scale 0: nothing is launched for the image term
    unet.set_ip_adapter_scale(1.0)
    assert torch.equal(run(ip_image_embeds=embd), on)
    assert torch.equal(run(), plain)                                               # no image context: the plain forward
    lib = _lib.load()
    unet.set_ip_context(embd)
    assert lib.ladi_unet_clear_ip_context(unet.h) == 0
    unet._ip_key = "none"
    assert torch.equal(run(), plain)


def test_forward_tokens_and_pag(tiny):
    """set_ip_tokens with N = 16 on an adapter loaded with N = 4; PAG and the image term in one forward; the rows form (sample0)"""
    unet, hw = tiny["mod"]["unet"], (32, 24)
    x, ehs, xd, ed, emb, embd = _fwd_inputs(tiny, hw)
    tok16 = torch.randn((4, 16, tiny["ucfg"]["cross_attention_dim"]), generator=torch.Generator().manual_seed(5)).half().float()
    got = unet(xd, T0, encoder_hidden_states=ed, ip_tokens=tok16.to(U.dev())).sample.float().cpu()
    _close("IP forward, 16 given tokens", got, RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, ip=(tiny["ip"], tok16, ONES)),
           "ip_forward_tiny_tokens16")
    names = ["down.block_1", "mid", "up.block_2"]
    unet.set_pag_applied_layers(names)
    tok = R.image_proj(tiny["ip"], emb)
    both = unet(xd, T0, encoder_hidden_states=ed, pag_first=2, ip_image_embeds=embd).sample.float().cpu()
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, pag=(PG.layer_prefixes(names), 2), ip=(tiny["ip"], tok, ONES))
    _close("IP + PAG forward", both, ref, "ip_forward_tiny_pag")
    sub = unet(xd[2:].contiguous(), T0, encoder_hidden_states=ed, sample0=2, pag_first=2, ip_image_embeds=embd).sample.float().cpu()
    _close("IP + PAG forward, rows [2, 4)", sub, ref[2:])


def test_forward_measurement_route(tiny, lib):
    """ladi_unet_set_ip_route(1), the A/B arm of tools/bench_ip_adapter.py (flash attention over the image keys into scratch + a scaled add),
    meets the same reference at the same thresholds; route 0 afterwards gives the shipped route's bits again"""
    unet, hw = tiny["mod"]["unet"], (26, 19)
    x, ehs, xd, ed, emb, embd = _fwd_inputs(tiny, hw)
    run = lambda: unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=embd).sample.float().cpu()
    on = run()
    assert lib.ladi_unet_set_ip_route(unet.h, 2) == -1 and lib.ladi_unet_set_ip_route(unet.h, 1) == 0
    try:
        alt = run()
    finally:
        assert lib.ladi_unet_set_ip_route(unet.h, 0) == 0
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, ip=(tiny["ip"], R.image_proj(tiny["ip"], emb), ONES))
    _close("IP forward by flash + add", alt, ref)
    assert torch.equal(run(), on)


def test_forward_misuse(tiny, lib):
    unet, hw = tiny["mod"]["unet"], (32, 24)
    x, ehs, xd, ed, emb, embd = _fwd_inputs(tiny, hw)
    plain = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    with pytest.raises(_lib.NativeError, match="batch mismatch"):
        unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=embd[:3].contiguous())
    with pytest.raises(ValueError, match="embedding width"):
        unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=torch.zeros((4, E + 8), device=U.dev()))
    with pytest.raises(ValueError, match="cannot both"):
        unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=embd, ip_tokens=embd)
    with pytest.raises(ValueError, match="ip_tokens has shape"):
        unet(xd, T0, encoder_hidden_states=ed, ip_tokens=torch.zeros((4, 65, 128), device=U.dev()))
    bad = (ctypes.c_float * 16)(*([1.0] * 15 + [float("nan")]))
    unet.set_ip_adapter_scale({"down": 0.5})
    before = unet.ip_adapter_scale
    assert lib.ladi_unet_set_ip_scale(unet.h, bad, 16) == -1 and "not finite" in _lib.last_error()
    assert lib.ladi_unet_set_ip_scale(unet.h, bad, 15) == -1 and "16 scales" in _lib.last_error()
    assert unet.ip_adapter_scale == before
    with pytest.raises(_lib.NativeError, match="already loaded"):
        unet.load_ip_adapter(dict(tiny["ip"]))
    assert torch.equal(unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu(), plain)


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 4
CUTOFF = [7.5, 7.5, 1.0, 1.0]
LAYERS = ("down.block_1", "up.block_2")
CASES = {
    "plain": dict(ip=False),
    "base": dict(),
    "half": dict(scales=0.5),
    "pndm": dict(scheduler="pndm", neg=True),
    "nocfg": dict(guidance=1.0),
    "cutoff": dict(table=CUTOFF, neg=True),
    "feature_cache": dict(feature_cache=2),
    "pag": dict(pag_scale=3.0, layers=LAYERS),
    "callback": dict(callback=lambda i, lat: _edit(lat)),
}


def _edit(lat):
    return lat * 0.8


def _scales(kw):
    return [float(kw.get("scales", 1.0))] * 16


def _ref(tiny, case):
    if case not in tiny["ref"]:
        kw = dict(CASES[case])
        ip = (tiny["ip"], tiny["emb"], tiny["neg"] if kw.get("neg") else None, _scales(kw)) if kw.get("ip", True) else None
        counts = {}
        a = (tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], TT.inputs(tiny, 2, 64, 48))
        img, lat = RT.tryon_reference(*a, STEPS, kw.get("scheduler", "ddim"), ip=ip, pag=(kw.get("pag_scale", 0.0), 0.0, kw.get("layers", ("mid",))),
                                      guidance=kw.get("guidance", 7.5), table=kw.get("table"), callback=kw.get("callback"),
                                      feature_cache=(kw.get("feature_cache"), 0), cloth_cond_rate=None, info=counts)
        tiny["ref"][case] = (img, lat, counts)
    return tiny["ref"][case]


def _call(tiny, pipe, case, fused=True, graph=True, **over):
    kw = dict(CASES[case])
    inp, d = TT.inputs(tiny, 2, 64, 48), U.dev()
    pipe.set_pag_applied_layers(list(kw.get("layers", ("mid",))))
    pipe.set_ip_adapter_scale(kw.get("scales", 1.0))
    cb = None
    if kw.get("callback"):
        def cb(i, t, lat):
            lat.copy_(_edit(lat))
    args = dict(guidance_scale=kw.get("table", kw.get("guidance", 7.5)), pag_scale=kw.get("pag_scale", 0.0), feature_cache=kw.get("feature_cache"),
                callback=cb)
    if kw.get("ip", True):
        args.update(ip_adapter_image_embeds=tiny["emb"].to(d), negative_ip_adapter_image_embeds=tiny["neg"].to(d) if kw.get("neg") else None)
    args.update(over)
    return TT.call(tiny, pipe, inp, fused, graph, num_inference_steps=STEPS, **args)


def _run(tiny, case, arm):
    """one run per (case, arm) on a fresh pipeline (a fresh native handle), shared by the tests below"""
    if (case, arm) not in tiny["run"]:
        pipe = TT.pipe(tiny, CASES[case].get("scheduler", "ddim"))
        img, lat = _call(tiny, pipe, case, fused=arm != "modular", graph=arm == "graph")
        tiny["run"][(case, arm)] = (img, lat, pipe.cond_only_evals() if arm != "modular" else None)
    return tiny["run"][(case, arm)]


@pytest.mark.parametrize("arm", ["graph", "eager", "modular"])
def test_loop_vs_reference(tiny, arm):
    """thresholds of test_tryon_pipeline_tiny (latents >= 40 dB, image >= 35 dB) against ref_tryon.tryon_reference, a NULL negative
    (zeros through the projection); below 40 dB against the plain reference"""
    ref_img, ref_lat, _ = _ref(tiny, "base")
    img, lat, _ = _run(tiny, "base", arm)
    p_img, p_lat = TT.assert_close("tiny IP %s" % arm, img, lat, ref_img, ref_lat)
    U.record_parity("ip_tiny_ddim_%s" % arm, dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    p = U.psnr(lat, _ref(tiny, "plain")[1])
    print("tiny IP %s against the plain reference: latents %.2f dB" % (arm, p))
    assert p < 40.0, p


def test_graph_equals_eager_bitwise(tiny):
    img_g, lat_g, _ = _run(tiny, "base", "graph")
    img_e, lat_e, _ = _run(tiny, "base", "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)


@pytest.mark.parametrize("arm", ["graph", "modular"])
@pytest.mark.parametrize("case", ["pndm", "nocfg", "cutoff", "feature_cache", "pag", "callback"])
def test_loop_cases_vs_reference(tiny, case, arm):
    """PNDM with given negatives; guidance_scale = 1 ([pos] alone); a guidance schedule with a cond-only tail; the feature cache; PAG (a third
    group with the cond group's image tokens); a callback that edits the latents"""
    ref_img, ref_lat, counts = _ref(tiny, case)
    img, lat, n_cond = _run(tiny, case, arm)
    p_img, p_lat = TT.assert_close("tiny IP %s %s" % (case, arm), img, lat, ref_img, ref_lat)
    U.record_parity("ip_tiny_%s_%s" % (case, arm), dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    if arm == "graph":
        assert n_cond == counts["cond_only"], (n_cond, counts)
        img_e, lat_e, _ = _run(tiny, case, "eager")
        assert torch.equal(lat, lat_e) and torch.equal(img, img_e)
    if case == "cutoff":
        assert counts["cond_only"] == 2
    if case == "nocfg":
        assert counts["cond_only"] == STEPS
    if case == "feature_cache":
        assert counts["shallow"] == 2


def test_lanes_match_single_lane(tiny):
    """two sample-group lanes against one: latents >= 45 dB, the threshold of test_unet_lanes_match_single_lane"""
    _, lat_1, _ = _run(tiny, "base", "graph")
    pipe = TT.pipe(tiny)
    pipe.lanes = 2
    _, lat_2 = _call(tiny, pipe, "base")
    assert pipe.lib_lanes() == 2
    assert U.psnr(lat_2, _ref(tiny, "base")[1]) >= 40.0
    p = U.psnr(lat_2, lat_1)
    print("IP two lanes against one: latents %.2f dB" % p)
    assert p >= 45.0, p


def test_no_stale_graph(tiny):
    """one pipeline with use_graph: plain -> scale 1 -> scale 0.5 -> scale 0 -> image prompt off.  Every image run meets its own reference
    and equals the eager run of a fresh pipeline bit for bit, the two are further apart than the threshold, scale 0 and off are the plain run"""
    pipe = TT.pipe(tiny)
    img_1, lat_1 = _call(tiny, pipe, "plain")
    img_2, lat_2 = _call(tiny, pipe, "base")
    img_3, lat_3 = _call(tiny, pipe, "half")
    img_4, lat_4 = _call(tiny, pipe, "base", ip_adapter_image_embeds=tiny["emb"].to(U.dev()))
    pipe.set_ip_adapter_scale(0.0)
    inp, d = TT.inputs(tiny, 2, 64, 48), U.dev()
    zero = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
                warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
                negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=64, width=48, num_inference_steps=STEPS, output_type="np",
                noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), ip_adapter_image_embeds=tiny["emb"].to(d))
    lat_0 = pipe.last_latents.float().cpu()
    img_5, lat_5 = _call(tiny, pipe, "plain")
    TT.assert_close("plain", img_1, lat_1, *_ref(tiny, "plain")[:2])
    TT.assert_close("IP 1.0", img_2, lat_2, *_ref(tiny, "base")[:2])
    TT.assert_close("IP 0.5", img_3, lat_3, *_ref(tiny, "half")[:2])
    assert torch.equal(lat_2, _run(tiny, "base", "eager")[1]) and torch.equal(lat_3, _run(tiny, "half", "eager")[1])
    assert torch.equal(lat_4, lat_2) and torch.equal(img_4, img_2)
    p = U.psnr(lat_2, lat_3)
    print("IP runs at scale 1.0 / 0.5: latents %.2f dB apart" % p)
    assert p < 40.0, p
    assert torch.equal(lat_0, lat_1) and torch.equal(torch.from_numpy(zero.images), img_1)        # every scale 0: the plain run bit for bit
    assert torch.equal(lat_5, lat_1) and torch.equal(img_5, img_1)


def test_misuse_fails_before_anything_is_launched(tiny, lib):
    """wrong E, wrong batch, negatives alone, and -- at the C boundary -- a run on a UNet without a loaded adapter: an error with a message,
    and the next plain run on the same handle is the plain run.  Then the adapter is loaded again, from module-named keys"""
    pipe, unet = TT.pipe(tiny), tiny["mod"]["unet"]
    img_1, lat_1 = _call(tiny, pipe, "plain")
    d = U.dev()
    with pytest.raises(ValueError, match="width %d" % (E + 8)):
        _call(tiny, pipe, "base", ip_adapter_image_embeds=torch.zeros((2, E + 8), device=d))
    with pytest.raises(ValueError, match="batch 3"):
        _call(tiny, pipe, "base", ip_adapter_image_embeds=torch.zeros((3, E), device=d))
    with pytest.raises(ValueError, match="without `ip_adapter_image_embeds`"):
        _call(tiny, pipe, "plain", negative_ip_adapter_image_embeds=torch.zeros((2, E), device=d))
    # diffusers' list form with the negatives first is the run with given negatives
    both = [torch.cat([tiny["neg"], tiny["emb"]])[:, None].to(d)]
    _, lat_l = _call(tiny, pipe, "base", ip_adapter_image_embeds=both)
    _, lat_n = _call(tiny, pipe, "base", negative_ip_adapter_image_embeds=tiny["neg"].to(d))
    assert torch.equal(lat_l, lat_n) and not torch.equal(lat_l, _run(tiny, "base", "graph")[1])
    fwd = _fwd_inputs(tiny, (32, 24))
    on = unet(fwd[2], T0, encoder_hidden_states=fwd[3], ip_image_embeds=fwd[5]).sample.float().cpu()
    plain_fwd = unet(fwd[2], T0, encoder_hidden_states=fwd[3]).sample.float().cpu()
    unet.set_ip_context(fwd[5])                                                    # unload drops a set image context too
    unet.unload_ip_adapter()
    try:
        assert unet.ip_adapter_info is None
        assert torch.equal(unet(fwd[2], T0, encoder_hidden_states=fwd[3]).sample.float().cpu(), plain_fwd)
        with pytest.raises(ValueError, match="load_ip_adapter"):
            _call_plain_after_unload(tiny, pipe, ip_adapter_image_embeds=tiny["emb"].to(d))
        with pytest.raises(ValueError, match="load_ip_adapter"):
            unet(fwd[2], T0, encoder_hidden_states=fwd[3], ip_image_embeds=fwd[5])
        inp = TT.inputs(tiny, 2, 64, 48)
        a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
             inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], 64, 48, STEPS, 7.5, 1.0, False, True)
        e16 = tiny["emb"].to(d).half().contiguous()
        with pytest.raises(_lib.NativeError, match="no IP-Adapter loaded"):
            pipe._run_fused(*a, ip=(e16, torch.zeros_like(e16)))
        one = (ctypes.c_float * 16)(*ONES)
        assert lib.ladi_unet_set_ip_scale(unet.h, one, 16) == -1 and "no IP-Adapter" in _lib.last_error()
        assert lib.ladi_unet_set_ip_context(unet.h, ctypes.c_void_p(e16.data_ptr()), 2, stream_ptr()) != 0
        img_2, lat_2 = _call_plain_after_unload(tiny, pipe)
        assert torch.equal(lat_2, lat_1) and torch.equal(img_2, img_1)             # after unload: the plain run bit for bit
    finally:
        unet.load_ip_adapter(R.to_diffusers(tiny["ip"], 2, numbered=False))
    assert unet.ip_adapter_scale == ONES
    assert torch.equal(unet(fwd[2], T0, encoder_hidden_states=fwd[3], ip_image_embeds=fwd[5]).sample.float().cpu(), on)


def _call_plain_after_unload(tiny, pipe, **over):
    """the plain case without touching the (unloaded) adapter's scales"""
    inp, d = TT.inputs(tiny, 2, 64, 48), U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=64, width=48, num_inference_steps=STEPS, output_type="np",
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **over)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()
