"""Perturbed-attention guidance on the device: the identity-attention copy kernel on strided views in poisoned buffers, the step and
statistics kernels with the third sample group against tests/pag_ref.py, the native UNet's forward with perturbed samples against the
reference forward, then the tiny model end to end (fused hipGraph, fused eager, modular, lanes, with the other sampler switches) against
ref_tryon.tryon_reference, the graph key and the misuse."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import pipeline as P
from tests import guidance_ref as G
from tests import pag_ref as R
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import tiny_tryon as TT
from tests import util as U
from tests.test_gpu_guidance import SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ identity operator
def _qkv(rows, Cc, seed):
    """a fused QKV buffer [rows, 3C] whose Q and K thirds hold NaN and whose V third holds data (with a few special values)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((rows, 3 * Cc), float("nan"), dtype=torch.float16)
    v = (torch.randn((rows, Cc), generator=g) * 4).half()
    v[0, 0], v[-1, -1], v[0, -1] = float("inf"), -0.0, 6.0e-8
    t[:, 2 * Cc:] = v
    return t, v


@pytest.mark.parametrize("rows,Cc", [(1, 64), (5, 64), (48, 128), (768, 64), (3, 1280)])
def test_identity_op(lib, rows, Cc):
    """O = V: the output bits are the source bits, nothing outside the two views changes, two launches are bit-equal"""
    t, v = _qkv(rows, Cc, rows + Cc)
    gq = U.guarded(t)
    outs = []
    for _ in range(2):
        go = U.guarded_out(rows, Cc, ld=Cc + 8)
        rc = lib.ladi_op_pag_identity(ctypes.c_void_p(gq.col(2 * Cc)), 3 * Cc, ctypes.c_void_p(go.ptr), go.ld, rows, Cc, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        assert torch.equal(_bits(go.cpu()), _bits(v))
        U.assert_untouched(go, "pag_identity o")
        outs.append(_bits(go.cpu()))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(_bits(gq.cpu()), _bits(t))            # the source (and its Q / K thirds) is read only
    U.assert_untouched(gq, "pag_identity qkv")


def test_identity_op_refusals(lib):
    """C = 12, a misaligned base, a stride below C and null pointers: an error with a message, nothing written"""
    rows, Cc = 4, 16
    t, v = _qkv(rows, Cc, 1)
    gq, go = U.guarded(t), U.guarded_out(rows, Cc, ld=Cc + 8)
    before = _bits(go.buf.cpu())
    V, O = gq.col(2 * Cc), go.ptr
    run = lambda v_, ldv, o_, ldo, r, c: lib.ladi_op_pag_identity(ctypes.c_void_p(v_) if v_ else None, ldv, ctypes.c_void_p(o_) if o_ else None,
                                                                  ldo, r, c, stream_ptr())
    assert run(V, 3 * Cc, O, go.ld, rows, 12) != 0 and "C = 12" in _lib.last_error()
    assert run(V + 2, 3 * Cc, O, go.ld, rows, 8) != 0 and "aligned" in _lib.last_error()
    assert run(V, 3 * Cc, O + 2, go.ld, rows, 8) != 0 and "aligned" in _lib.last_error()
    assert run(V, 8, O, go.ld, rows, Cc) != 0 and "stride" in _lib.last_error()
    assert run(V, 3 * Cc, O, Cc + 4, rows, Cc) != 0
    assert run(None, 3 * Cc, O, go.ld, rows, Cc) != 0 and "null" in _lib.last_error()
    assert run(V, 3 * Cc, None, go.ld, rows, Cc) != 0 and "null" in _lib.last_error()
    assert run(V, 3 * Cc, O, go.ld, 0, Cc) != 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(go.buf.cpu()), before)


# ------------------------------------------------------------------------------------------------------------------ step kernel
def _mirror(kind):
    import ladi_vton_amd as L
    return {"ddim": L.DDIMScheduler, "pndm": L.PNDMScheduler, "dpmpp2m": L.DPMSolverMultistepScheduler,
            "euler_a": L.EulerAncestralDiscreteScheduler}[kind]()


def _tables(name, n):
    """-> (guidance table, PAG table).  adaptive: positive scales, then zeros.  mixed, with a guidance cut-off pattern: CFG + PAG (0, 6),
    cond-only + PAG (1, 4), CFG without PAG (2, 5), cond-only without PAG (3), then CFG + PAG"""
    if name == "const":
        return [7.5] * n, [3.0] * n
    if name == "adaptive":
        return [7.5] * n, ([3.0, 1.755, 0.505] + [0.0] * n)[:n]
    return ([7.5, 1.0, 7.5, 1.0, 0.5, 9.0, 2.0] + [3.0] * n)[:n], ([3.0, 2.0, 0.0, 0.0, 1.5, 0.0, 2.5] + [1.0] * n)[:n]


def _sched_case(kind, B, h, w, cfg, name, seed=67):
    sch = _mirror(kind)
    steps = 8
    sch.set_timesteps(steps)
    n = len(sch.timesteps)
    gtab, ptab = _tables(name, n)
    hw, groups = h * w, 3 if cfg else 2
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((n, groups * B, hw, 4), generator=g).half()
    for i in range(n):
        if cfg and not G.is_cfg(gtab[i]):
            eps[i, :B] = float("nan")              # a cond-only evaluation never reads its uncond rows
        if not ptab[i] > 0.0:
            eps[i, (groups - 1) * B:] = float("nan")   # an evaluation without PAG never reads its perturbed rows
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    noise = torch.stack([torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(17 + i)) for i in range(n)])
    return sch, steps, n, gtab, ptab, eps, lat0, noise


def _run_pag(lib, sch, steps, n, cfg, gtab, ptab, eps_ptr, ld, B, hw, phi, lat0, noise):
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = noise.contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    gt = (ctypes.c_float * n)(*gtab) if cfg else None
    pt = (ctypes.c_float * n)(*ptab)
    rc = lib.ladi_op_sched_run_pag(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, eps_ptr, ld, n, B, hw, 1 if cfg else 0, gt, pt, phi, ptr(L_),
                                   ptr(N), n, stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return L_


@pytest.mark.parametrize("cfg,phi", [(1, 0.0), (1, 0.7), (0, 0.0)])
@pytest.mark.parametrize("name", ["const", "adaptive", "mixed"])
@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["ddim", "pndm", "dpmpp2m", "euler_a"])
def test_sched_run_pag_vs_reference(lib, kind, B, h, w, name, cfg, phi, monkeypatch):
    """the step kernel with the third group over a random eps sequence against the scheduler mirror with pag_ref's combine: rel-L2 < 1e-5,
    the bound of test_sched_run_guided_vs_reference; rows an evaluation must not read hold NaN and the result is finite"""
    import ladi_vton_amd.schedulers as S
    sch, steps, n, gtab, ptab, eps, lat0, noise = _sched_case(kind, B, h, w, cfg, name)
    hw = h * w
    draws = iter(noise)
    monkeypatch.setattr(S, "_step_noise", lambda shape, dtype, generator, device: next(draws).to(dtype))
    e_nchw = eps.view(n, eps.shape[1], h, w, 4).permute(0, 1, 4, 2, 3)
    ref = R.sched_reference(sch, e_nchw, cfg, gtab, ptab, phi, lat0)
    E = eps.to(U.dev())
    got = _run_pag(lib, sch, steps, n, cfg, gtab, ptab, ptr(E), 4, B, hw, phi, lat0, noise).cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    err = U.rel_l2(got, ref)
    print("sched_run_pag %s B=%d hw=%d %s cfg=%d phi=%.1f: rel-L2 %.3g" % (kind, B, hw, name, cfg, phi, err))
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    assert err < 1e-5, err


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["ddim", "pndm", "dpmpp2m", "euler_a"])
def test_sched_run_pag_zero_table_is_the_guided_run_bitwise(lib, kind, B, h, w, phi):
    """an all-zero PAG table (the perturbed rows hold NaN) equals ladi_op_sched_run_guided over the first 2B rows, bit for bit"""
    sch, steps, n, gtab, _, eps, lat0, noise = _sched_case(kind, B, h, w, 1, "mixed")
    hw = h * w
    eps[:, 2 * B:] = float("nan")
    E = eps.to(U.dev())
    got = _run_pag(lib, sch, steps, n, 1, gtab, [0.0] * n, ptr(E), 4, B, hw, phi, lat0, noise)
    E2 = eps[:, :2 * B].contiguous().to(U.dev())
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    N = noise.contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    rc = lib.ladi_op_sched_run_guided(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, ptr(E2), 4, n, B, hw, (ctypes.c_float * n)(*gtab), phi,
                                      ptr(L_), ptr(N), n, stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, L_)


@pytest.mark.parametrize("cfg", [1, 0])
def test_sched_run_pag_strided_matches_dense(lib, cfg):
    """ld_eps = 8 between poisoned lanes, a mixed table, phi > 0: bit-equal to the dense run, lanes 4..7 and the rows around are never read"""
    B, h, w = SHAPES[1]
    sch, steps, n, gtab, ptab, eps, lat0, noise = _sched_case("ddim", B, h, w, cfg, "mixed")
    phi = 0.7 if cfg else 0.0
    E = eps.to(U.dev())
    dense = _run_pag(lib, sch, steps, n, cfg, gtab, ptab, ptr(E), 4, B, h * w, phi, lat0, noise)
    ge = U.guarded(eps.reshape(-1, 4), ld=8)
    strided = _run_pag(lib, sch, steps, n, cfg, gtab, ptab, ctypes.c_void_p(ge.ptr), 8, B, h * w, phi, lat0, noise)
    assert torch.isfinite(dense).all() and torch.equal(dense, strided)
    U.assert_untouched(ge, "sched_run_pag eps")


# ------------------------------------------------------------------------------------------------------------------ statistics kernel
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_cfg_stats_pag_vs_reference(lib, B, h, w, ld):
    """factor[b] with the three-term guided sum against float64 over the same fp16 values: relative error <= 1e-5, the bound of
    test_cfg_stats_vs_reference; two calls are bit-equal; scale 0 is ladi_op_cfg_stats bit for bit and never reads the perturbed rows"""
    hw, gs, s, phi = h * w, 7.5, 3.0, 0.7
    g = torch.Generator().manual_seed(5)
    eu = torch.randn((B, hw, 4), generator=g) * 0.8 + 0.05
    ec = torch.randn((B, hw, 4), generator=g) * (torch.arange(B).view(B, 1, 1) * 0.3 + 0.6) - 0.1
    ep = ec + torch.randn((B, hw, 4), generator=g) * 0.3
    eps = torch.cat([eu, ec, ep]).half()
    ge = U.guarded(eps.reshape(3 * B * hw, 4), ld=ld)
    e64 = eps.double()
    ref = G.rescale_factor(R.guided_eps(e64[:B], e64[B:2 * B], e64[2 * B:], gs, s), e64[B:2 * B], phi).reshape(B)
    out = torch.full((2, B + 2), -7.0, device=U.dev())
    for k in range(2):
        assert lib.ladi_op_cfg_stats_pag(ctypes.c_void_p(ge.ptr), ld, B, hw, gs, s, phi, ptr(out[k]), stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    rel = ((got[0, :B].double() - ref) / ref).abs().max().item()
    print("cfg_stats_pag B=%d hw=%d ld=%d: max rel err %.3g, factors %s" % (B, hw, ld, rel, got[0, :B].tolist()))
    assert torch.isfinite(got[0, :B]).all() and rel <= 1e-5, rel
    assert torch.equal(got[0], got[1]) and (got[:, B:] == -7.0).all()
    plain = G.rescale_factor(G.guided_eps(e64[:B], e64[B:2 * B], gs), e64[B:2 * B], phi).reshape(B)
    assert ((ref - plain) / plain).abs().max().item() > 1e-3            # the third term is visible at the bound
    U.assert_untouched(ge, "cfg_stats_pag eps")
    eps[2 * B:] = float("nan")
    gz = U.guarded(eps.reshape(3 * B * hw, 4), ld=ld)
    z = torch.full((2, B), -7.0, device=U.dev())
    assert lib.ladi_op_cfg_stats_pag(ctypes.c_void_p(gz.ptr), ld, B, hw, gs, 0.0, phi, ptr(z[0]), stream_ptr()) == 0, _lib.last_error()
    assert lib.ladi_op_cfg_stats(ctypes.c_void_p(gz.ptr), ld, B, hw, gs, phi, ptr(z[1]), stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.equal(z[0], z[1])


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481
LAYER_SETS = {"mid": "mid", "outer": ["down.block_0.attentions_1", "up.block_3"], "inner": ["down.block_1", "up.block_2"],
              "all": ["down", "mid", "up"]}


@pytest.fixture(scope="module")
def tiny():
    t = TT.build()
    yield t
    t["mod"]["unet"].set_pag_applied_layers("mid")
    t["mod"]["unet"].disable_freeu()


@pytest.fixture(autouse=True)
def _defaults_between_tests(request):
    """the layer mask and FreeU are sticky in the native UNet the tests of this module share: every test starts and ends with the defaults"""
    yield
    if "tiny" in request.fixturenames:
        u = request.getfixturevalue("tiny")["mod"]["unet"]
        u.set_pag_applied_layers("mid")
        u.disable_freeu()


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
@pytest.mark.parametrize("which", list(LAYER_SETS))
def test_forward_vs_reference(tiny, which, hw):
    """NativeUNet tiny, n = 4, t = 481, pag_first = 2.  Thresholds of test_unet_forward_tiny (PSNR >= 55 dB, rel-L2 <= 5e-3) against
    ref_unet.unet_forward; samples 0, 1 keep the plain forward's bits (one attention workgroup per (sample, head, query tile)); samples 2, 3
    are another function than the plain forward; the default layers give the earlier bits again"""
    unet, names = tiny["mod"]["unet"], LAYER_SETS[which]
    x, ehs, xd, ed = TT.unet_inputs(tiny, hw)
    run = lambda **kw: unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu()
    plain = run()
    mid_before = run(pag_first=2)
    unet.set_pag_applied_layers(names)
    assert unet.pag_applied_layers == R.mask_of(R.layer_prefixes(names))
    on = run(pag_first=2)
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, pag=(R.layer_prefixes(names), 2))
    ps, rl, pp = U.psnr(on, ref), U.rel_l2(on, ref), U.psnr(on[2:], plain[2:])
    print("PAG forward %s %dx%d: PSNR %.2f dB, rel-L2 %.3g; perturbed samples against plain %.2f dB" % ((which,) + hw + (ps, rl, pp)))
    U.record_parity("pag_forward_tiny_%s_%dx%d" % ((which,) + hw), dict(psnr_db=round(ps, 2), rel_l2=rl, vs_plain_db=round(pp, 2)))
    assert on.shape == ref.shape and torch.isfinite(on).all()
    assert ps >= 55.0 and rl <= 5e-3, (ps, rl)
    assert torch.equal(on[:2], plain[:2])
    assert pp < 55.0, pp
    assert torch.equal(run(pag_first=4), plain)                  # pag_first = n: the plain forward bit for bit
    assert torch.equal(run(pag_first=2), on)
    unet.set_pag_applied_layers("mid")
    assert unet.pag_applied_layers == 1 << 6
    assert torch.equal(run(pag_first=2), mid_before) and torch.equal(run(), plain)


@pytest.mark.parametrize("n,first", [(4, 0), (3, 1)])
def test_forward_other_splits(tiny, n, first):
    """pag_first = 0: every sample perturbed, the selected blocks launch no self-attention; pag_first = 1 of n = 3: an odd split"""
    unet, names = tiny["mod"]["unet"], LAYER_SETS["all"]
    x, ehs, xd, ed = TT.unet_inputs(tiny, (32, 24), n)
    unet.set_pag_applied_layers(names)
    on = unet(xd, T0, encoder_hidden_states=ed, pag_first=first).sample.float().cpu()
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, pag=(R.layer_prefixes(names), first))
    ps, rl = U.psnr(on, ref), U.rel_l2(on, ref)
    print("PAG forward all blocks n = %d, pag_first = %d: PSNR %.2f dB, rel-L2 %.3g" % (n, first, ps, rl))
    U.record_parity("pag_forward_tiny_all_n%d_first%d" % (n, first), dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert torch.isfinite(on).all() and ps >= 55.0 and rl <= 5e-3, (ps, rl)
    # the rows form: samples [1, n) of the same context (all of them perturbed) meet those rows of the reference at the same thresholds
    if first:
        sub = unet(xd[1:].contiguous(), T0, encoder_hidden_states=ed, sample0=1, pag_first=first).sample.float().cpu()
        assert U.psnr(sub, ref[1:]) >= 55.0 and U.rel_l2(sub, ref[1:]) <= 5e-3, (U.psnr(sub, ref[1:]), U.rel_l2(sub, ref[1:]))


def test_layer_setter_misuse(tiny, lib):
    unet = tiny["mod"]["unet"]
    assert lib.ladi_unet_pag_layer_count(unet.h) == 16
    assert lib.ladi_unet_set_pag_layers(unet.h, 0) == -1 and "selects no transformer block" in _lib.last_error()
    assert lib.ladi_unet_set_pag_layers(unet.h, 1 << 16) == -1 and "16 blocks" in _lib.last_error()
    with pytest.raises(_lib.NativeError):
        unet.set_pag_applied_layers(0)
    with pytest.raises(ValueError):
        unet.set_pag_applied_layers("down.block_3")
    assert unet.pag_applied_layers == 1 << 6
    x, ehs, xd, ed = TT.unet_inputs(tiny, (32, 24))
    with pytest.raises(ValueError, match="feature_cache"):
        unet(xd, T0, encoder_hidden_states=ed, pag_first=2, feature_cache="capture")
    with pytest.raises(ValueError, match="pag_first"):
        unet(xd, T0, encoder_hidden_states=ed, pag_first=-1)


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 4
LAYERS = ("down.block_1", "up.block_2")
LAYERS_B = ("down.block_0", "up.block_3")
FREEU = (0.9, 0.2, 1.4, 1.6)
CUTOFF = [7.5, 7.5, 1.0, 1.0]


def _edit(lat):
    return lat * 0.8


# the keywords of one case: the reference's (_ref hands them to ref_tryon.tryon_reference) and, under "pipe", what the pipeline call gets instead
CASES = {
    "plain": dict(pag_scale=0.0),
    "base": dict(pag_scale=3.0),
    "scale1": dict(pag_scale=1.0),
    "layers_b": dict(pag_scale=3.0, layers=LAYERS_B),
    "pndm": dict(pag_scale=3.0, scheduler="pndm"),
    "nocfg": dict(pag_scale=3.0, guidance=1.0),
    "adaptive": dict(pag_scale=3.0, pag_adaptive_scale=0.005),
    "cutoff": dict(pag_scale=3.0, table=CUTOFF),
    "rescale": dict(pag_scale=3.0, phi=0.7),
    "freeu": dict(pag_scale=3.0, freeu=FREEU),
    "preserve": dict(pag_scale=3.0, preserve_latents=True),
    "callback": dict(pag_scale=3.0, callback=lambda i, lat: _edit(lat)),
    "mid128": dict(pag_scale=3.0, layers=("mid",), size=(128, 96)),
}


def _ref(tiny, case):
    if case not in tiny["ref"]:
        kw = dict(CASES[case])
        size = kw.pop("size", (64, 48))
        kw.setdefault("layers", LAYERS)
        counts = {}
        pag = (kw.pop("pag_scale"), kw.pop("pag_adaptive_scale", 0.0), kw.pop("layers"))
        preserve = ("latents", 0.0) if kw.pop("preserve_latents", False) else None
        img, lat = RT.tryon_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], TT.inputs(tiny, 2, *size),
                                      STEPS, kw.pop("scheduler", "ddim"), pag=pag, preserve=preserve, cloth_cond_rate=None, info=counts, **kw)
        tiny["ref"][case] = (img, lat, counts)
    return tiny["ref"][case]


def _call(tiny, pipe, case, fused=True, graph=True, **over):
    """one run of a case through the pipeline -> (images, latents)"""
    kw = dict(CASES[case])
    size = kw.pop("size", (64, 48))
    inp = TT.inputs(tiny, 2, *size)
    pipe.set_pag_applied_layers(list(kw.get("layers", LAYERS)))
    if kw.get("freeu"):
        pipe.enable_freeu(*kw["freeu"])
    else:
        pipe.disable_freeu()
    cb = None
    if kw.get("callback"):
        def cb(i, t, lat):
            lat.copy_(_edit(lat))
    args = dict(guidance_scale=kw.get("table", kw.get("guidance", 7.5)), guidance_rescale=kw.get("phi", 0.0), pag_scale=kw["pag_scale"],
                pag_adaptive_scale=kw.get("pag_adaptive_scale", 0.0), preserve_unmasked="latents" if kw.get("preserve_latents") else None,
                callback=cb)
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
    ref_img, ref_lat, counts = _ref(tiny, "base")
    img, lat, _ = _run(tiny, "base", arm)
    p_img, p_lat = TT.assert_close("tiny PAG %s" % arm, img, lat, ref_img, ref_lat)
    U.record_parity("pag_tiny_ddim_%s" % arm, dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    assert counts["pag"] == STEPS
    p = U.psnr(lat, _ref(tiny, "plain")[1])
    print("tiny PAG %s against the plain reference: latents %.2f dB" % (arm, p))
    assert p < 40.0, p                                        # and it is not the plain loop


def test_graph_equals_eager_bitwise(tiny):
    img_g, lat_g, _ = _run(tiny, "base", "graph")
    img_e, lat_e, _ = _run(tiny, "base", "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)


@pytest.mark.parametrize("arm", ["graph", "modular"])
@pytest.mark.parametrize("case", ["pndm", "nocfg", "adaptive", "cutoff", "rescale", "freeu", "preserve", "callback", "mid128"])
def test_loop_cases_vs_reference(tiny, case, arm):
    """PNDM; guidance_scale = 1 (two groups); an adaptive scale whose evaluations 2, 3 run without the perturbed group; a guidance cut-off
    (cond-only evaluations with PAG); guidance rescale on the three-term sum; FreeU; the latent blend; a callback that edits the latents (the
    re-import reaches the perturbed group); the default layer at 128x96"""
    ref_img, ref_lat, counts = _ref(tiny, case)
    img, lat, n_cond = _run(tiny, case, arm)
    p_img, p_lat = TT.assert_close("tiny PAG %s %s" % (case, arm), img, lat, ref_img, ref_lat)
    U.record_parity("pag_tiny_%s_%s" % (case, arm), dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    if arm == "graph":
        assert n_cond == counts["cond_only"], (n_cond, counts)
        img_e, lat_e, _ = _run(tiny, case, "eager")
        assert torch.equal(lat, lat_e) and torch.equal(img, img_e)
    if case == "adaptive":
        assert [s > 0.0 for s in counts["pag_table"]] == [True, True, False, False]
    if case == "cutoff":
        assert counts["cond_only"] == 2
    if case == "nocfg":
        assert counts["cond_only"] == STEPS


def test_lanes_match_single_lane(tiny):
    """two sample-group lanes (n = 6: the second holds one cond and both perturbed samples) against one: latents >= 45 dB, the threshold of
    test_unet_lanes_match_single_lane"""
    _, lat_1, _ = _run(tiny, "base", "graph")
    pipe = TT.pipe(tiny)
    pipe.lanes = 2
    _, lat_2 = _call(tiny, pipe, "base")
    assert pipe.lib_lanes() == 2
    assert U.psnr(lat_2, _ref(tiny, "base")[1]) >= 40.0
    p = U.psnr(lat_2, lat_1)
    print("PAG two lanes against one: latents %.2f dB" % p)
    assert p >= 45.0, p


def test_no_stale_graph(tiny):
    """one pipeline with use_graph: plain -> PAG 3.0 -> PAG 1.0 -> other layers -> pag_scale = 0.0.  The first and the last run are
    bit-equal (and equal a fresh plain run), every PAG run meets its own reference, and they are further apart than the threshold"""
    pipe = TT.pipe(tiny)
    img_1, lat_1 = _call(tiny, pipe, "plain")
    img_2, lat_2 = _call(tiny, pipe, "base")
    img_3, lat_3 = _call(tiny, pipe, "scale1")
    img_4, lat_4 = _call(tiny, pipe, "layers_b")
    img_5, lat_5 = _call(tiny, pipe, "base", pag_scale=0.0)
    assert torch.equal(lat_5, lat_1) and torch.equal(img_5, img_1)
    TT.assert_close("plain", img_1, lat_1, *_ref(tiny, "plain")[:2])
    TT.assert_close("PAG 3.0", img_2, lat_2, *_ref(tiny, "base")[:2])
    TT.assert_close("PAG 1.0", img_3, lat_3, *_ref(tiny, "scale1")[:2])
    TT.assert_close("PAG 3.0, other layers", img_4, lat_4, *_ref(tiny, "layers_b")[:2])
    for a, b, what in ((lat_2, lat_3, "3.0 / 1.0"), (lat_2, lat_4, "layers"), (lat_3, lat_4, "1.0 / layers")):
        p = U.psnr(a, b)
        print("PAG runs %s: latents %.2f dB apart" % (what, p))
        assert p < 40.0, (what, p)
    assert torch.equal(lat_2, _run(tiny, "base", "graph")[1])           # a fresh pipeline gives the same PAG run
    # the plain run of a pipeline that never saw PAG, through the keyword-less call
    inp, d = TT.inputs(tiny, 2, 64, 48), U.dev()
    out = TT.pipe(tiny)(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
                      warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
                      negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=64, width=48, num_inference_steps=STEPS,
                      output_type="np", noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    assert torch.equal(torch.from_numpy(out.images), img_1)


def test_misuse_fails_before_anything_is_launched(tiny, lib):
    """a PAG table of the wrong length, PAG together with a feature-cache plan, a bad table entry: an error with a message, and the next
    plain run on the same handle is the plain run"""
    pipe = TT.pipe(tiny)
    img_1, lat_1 = _call(tiny, pipe, "plain")
    inp, d = TT.inputs(tiny, 2, 64, 48), U.dev()
    a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
         inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], 64, 48, STEPS, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="PAG table has 3 entries, this run has 4 evaluations"):
        pipe._run_fused(*a, pag_table=[3.0] * 3)
    with pytest.raises(_lib.NativeError, match="feature-cache plan"):
        pipe._run_fused(*a, pag_table=[3.0] * STEPS, feature_cache=([1, 0, 1, 0], 0))
    pipe._run_fused(*a, pag_table=[0.0] * STEPS, feature_cache=([1, 0, 1, 0], 0))          # a table of zeros is no PAG
    with pytest.raises(ValueError, match="feature_cache"):
        _call(tiny, pipe, "base", feature_cache=2)
    h = pipe._tryon
    bad = (ctypes.c_float * 3)(3.0, -1.0, 2.0)
    assert lib.ladi_tryon_set_pag(h, bad, 3) == -1 and "entry 1" in _lib.last_error()
    nan = (ctypes.c_float * 2)(3.0, float("nan"))
    assert lib.ladi_tryon_set_pag(h, nan, 2) == -1
    assert lib.ladi_tryon_set_pag(h, None, 0) == 0
    img_2, lat_2 = _call(tiny, pipe, "plain")
    assert torch.equal(lat_2, lat_1) and torch.equal(img_2, img_1)
