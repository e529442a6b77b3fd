"""Self-attention guidance on the device: sag_map and sag_degrade on strided views in poisoned buffers against tests/sag_ref.py, the step
and statistics kernels with the degraded input's prediction, the native UNet's captured map against the reference inside its fp16 band,
then the tiny model end to end (fused hipGraph, fused eager, modular) against sag_ref.tryon_sag_reference with the device's masks forced,
the graph key, the refusals and one short run with each of the other switches."""
import ctypes
import math

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import guidance_ref as G
from tests import ip_adapter_ref as IPR
from tests import lora_ref as LR
from tests import sag_ref as S
from tests import tiny_tryon as TT
from tests import util as U
from tests.test_gpu_guidance import SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _vp(a):
    return ctypes.c_void_p(a)


# ------------------------------------------------------------------------------------------------------------------ sag_map operator
def _qk_case(n, T, H, seed):
    """fp16 Q, K [n, T, H * 64]: unit-variance rows; sample 0, head 0 has a row with one dominant key (logit ~ +60 against ~ 0) and, when there
    is a second key, a query / key pair whose logit reaches -60; the rest are ordinary logits of order 1"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((n, T, H * 64), generator=g)
    k = torch.randn((n, T, H * 64), generator=g)
    u = torch.zeros(64)
    u[:16] = 1.0                                       # |u|^2 = 16: (a u) . (b u) / 8 = 2 a b
    jq, jk = T // 2, T - 1
    q[0, jq, :64], k[0, jk, :64] = 5.5 * u, 5.5 * u    # logit 60.5
    if T > 1:
        k[0, 0, :64] = -5.5 * u                        # logit -60.5 for the same query
    return q.half(), k.half()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [1, 20])
@pytest.mark.parametrize("T", [1, 35, 48, 192, 300])
def test_sag_map_op(lib, T, H, n):
    """s against float64 on the same fp16 Q and K: tolerance 16 x the largest difference between a float32 torch evaluation and the float64
    one (another summation order at the same precision), floor 1e-5; m exact wherever the reference |s - 1| exceeds it; Q and K are column
    slices of a fused QKV buffer whose V third and surroundings hold NaN; two launches are bit-equal"""
    Cc = H * 64
    q, k = _qk_case(n, T, H, 1000 * T + 10 * H + n)
    fused = torch.full((n * T, 3 * Cc), float("nan"), dtype=torch.float16)
    fused[:, :Cc], fused[:, Cc:2 * Cc] = q.reshape(n * T, Cc), k.reshape(n * T, Cc)
    gq = U.guarded(fused, ld=3 * Cc + 8)
    s64 = S.col_sums(q.double(), k.double(), H)
    s32 = S.col_sums(q.float(), k.float(), H)
    tol = max(16.0 * float((s32.double() - s64).abs().max()), 1e-5)
    lg = torch.matmul(q[0, :, :64].double(), k[0, :, :64].double().t()) / 8.0
    assert float(lg.max()) >= 60.0 and (T == 1 or float(lg.min()) <= -60.0)   # the logits reach +-60: the maximum has to be subtracted
    outs = []
    for _ in range(2):
        gs = U.guarded_out(n, T, dtype=torch.float32, any_ld=True)
        mb = torch.full((n * T + 64,), 0xA5, dtype=torch.uint8, device=U.dev())
        rc = lib.ladi_op_sag_map(_vp(gq.col(0)), gq.ld, T * gq.ld, _vp(gq.col(Cc)), gq.ld, T * gq.ld, n, T, H, _vp(gs.ptr), _vp(mb.data_ptr() + 32),
                                 stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        s, m = gs.cpu(), mb[32:32 + n * T].cpu().reshape(n, T)
        assert bool((mb[:32] == 0xA5).all()) and bool((mb[32 + n * T:] == 0xA5).all())
        U.assert_untouched(gs, "sag_map s")
        outs.append((s, m))
    err = float((s.double() - s64).abs().max())
    print("sag_map T=%d H=%d n=%d: max |s - s64| %.3g, tolerance %.3g, s in [%.3g, %.3g]" % (T, H, n, err, tol, float(s64.min()), float(s64.max())))
    assert torch.isfinite(s).all() and err <= tol, (err, tol)
    pinned = (s64 - 1.0).abs() > tol
    assert torch.equal(m[pinned], S.mask_of(s64)[pinned]) and bool(((m == 0) | (m == 1)).all())
    assert torch.equal(m, S.mask_of(s))                                       # the mask is the threshold of the sums the kernel wrote
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(gq.cpu()[:, :2 * Cc].view(torch.int16), fused[:, :2 * Cc].view(torch.int16))
    U.assert_untouched(gq, "sag_map qkv")


def test_sag_map_op_refusals(lib):
    q, k = _qk_case(1, 8, 1, 3)
    Q, K = q.to(U.dev()), k.to(U.dev())
    s = torch.zeros((1, 8), device=U.dev())
    m = torch.zeros((1, 8), dtype=torch.uint8, device=U.dev())
    run = lambda *a: lib.ladi_op_sag_map(*a, stream_ptr())
    assert run(ptr(Q), 64, 512, ptr(K), 64, 512, 1, 8, 1, ptr(s), ptr(m)) == 0
    assert run(None, 64, 512, ptr(K), 64, 512, 1, 8, 1, ptr(s), ptr(m)) != 0 and "null" in _lib.last_error()
    assert run(ptr(Q), 64, 512, ptr(K), 64, 512, 1, 0, 1, ptr(s), ptr(m)) != 0
    assert run(ptr(Q), 60, 512, ptr(K), 64, 512, 1, 8, 1, ptr(s), ptr(m)) != 0 and "stride" in _lib.last_error()
    assert run(_vp(Q.data_ptr() + 2), 64, 512, ptr(K), 64, 512, 1, 7, 1, ptr(s), ptr(m)) != 0 and "aligned" in _lib.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ sag_degrade operator
DEGRADE_SIZES = [(5, 5, 2, 2), (6, 5, 3, 2), (8, 6, 1, 1), (8, 6, 3, 4), (13, 9, 2, 2), (13, 9, 4, 3), (64, 48, 8, 6), (64, 48, 5, 7)]


def _mask(kind, B, hm, wm):
    if kind == "zeros":
        return torch.zeros((B, hm, wm), dtype=torch.uint8)
    if kind == "ones":
        return torch.ones((B, hm, wm), dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(hm), torch.arange(wm), indexing="ij")
    return torch.stack([((yy + xx + b) % 2).to(torch.uint8) for b in range(B)])


@pytest.mark.parametrize("a", [0.9991, 0.0047])
@pytest.mark.parametrize("kind", ["zeros", "ones", "checker"])
@pytest.mark.parametrize("h,w,hm,wm", DEGRADE_SIZES)
def test_sag_degrade_op(lib, h, w, hm, wm, kind, a):
    """channels 0..3 of the B destination rows against sag_ref.degrade in float64.  Tolerance, from the magnitudes: the result is stored in
    fp16 (half a spacing of the reference) and computed in fp32 from terms of size L = max(|x| + 2 sqrt(1 - a) |b|) -- two 9-tap chains, the
    x0 arithmetic of every tap and the final sum, under 32 roundings of 2^-24 L.  The source rows' other channels are copied, the source
    rows, the rows of a third group and every pad row keep their bits"""
    B, hw = 2, h * w
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + hm)
    x = torch.randn((B, 4, h, w), generator=g) * (1.0 if a < 0.5 else 0.3)
    b = torch.randn((B, 4, h, w), generator=g).half().float()
    m = _mask(kind, B, hm, wm)
    sa, s1 = float(torch.tensor(math.sqrt(a), dtype=torch.float32)), float(torch.tensor(math.sqrt(1 - a), dtype=torch.float32))
    x64, b64 = x.double(), b.double()
    x0 = (x64 - s1 * b64) / sa
    Mk = S.upsampled(m, h, w).double()
    ref = sa * (S.blur9(x0) * Mk + x0 * (1 - Mk)) + s1 * b64
    Lmag = float((x64.abs() + 2 * s1 * b64.abs()).max())
    bound = 0.5 * U.ulp16(ref) + 32 * 2.0 ** -24 * Lmag
    lat = U.guarded(x.permute(0, 2, 3, 1).reshape(B * hw, 4).contiguous())
    ge = U.guarded(b.permute(0, 2, 3, 1).reshape(B * hw, 4).half(), ld=8)
    rows = torch.randn((3 * B * hw, 64), generator=g).half()
    rows[:, 31:] = 0
    rows[B * hw:] = float("nan")                                        # the destination group and a third group start as NaN
    gr = U.guarded(rows)
    M_ = m.to(U.dev())
    src, dst = gr.ptr, gr.ptr + B * hw * 64 * 2
    rc = lib.ladi_op_sag_degrade(_vp(lat.ptr), _vp(ge.ptr), 8, ptr(M_), B, h, w, hm, wm, sa, s1, 1.0, _vp(src), _vp(dst), 64, 64, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    out = gr.cpu()
    got = out[B * hw:2 * B * hw, :4].reshape(B, h, w, 4).permute(0, 3, 1, 2).double()
    err = (got - ref).abs()
    print("sag_degrade %dx%d map %dx%d %s a=%.4f: max err %.3g, bound there %.3g" % (h, w, hm, wm, kind, a, float(err.max()), float(bound.flatten()[err.argmax()])))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), float((err / bound).max())
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(out[B * hw:2 * B * hw, 4:]), bits(rows[:B * hw, 4:]))          # the base group's other channels
    assert torch.equal(bits(out[:B * hw]), bits(rows[:B * hw])) and torch.equal(bits(out[2 * B * hw:]), bits(rows[2 * B * hw:]))
    for gg, what in ((gr, "rows"), (lat, "latents"), (ge, "eps")):
        U.assert_untouched(gg, "sag_degrade " + what)
    if kind == "checker":
        assert float((got - x64).abs().max()) > 1e-3                      # the blur is visible
        # the same rows as source and destination (and no source): nothing but channels 0..3 changes
        for s_ in (src, None):
            g2 = U.guarded(rows[:B * hw])
            rc = lib.ladi_op_sag_degrade(_vp(lat.ptr), _vp(ge.ptr), 8, ptr(M_), B, h, w, hm, wm, sa, s1, 1.0, _vp(g2.ptr) if s_ else None, _vp(g2.ptr),
                                         64, 64, stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, _lib.last_error()
            o2 = g2.cpu()
            assert torch.equal(bits(o2[:, 4:]), bits(rows[:B * hw, 4:])) and torch.equal(bits(o2[:, :4]), bits(out[B * hw:2 * B * hw, :4]))
            U.assert_untouched(g2, "sag_degrade in place")


def test_sag_degrade_op_refuses_small_latents(lib):
    d = U.dev()
    x, e, m, o = torch.zeros((16, 4), device=d), torch.zeros((16, 4), dtype=torch.float16, device=d), torch.zeros((1, 1, 1), dtype=torch.uint8, device=d), torch.zeros((16, 4), dtype=torch.float16, device=d)
    for h, w in ((4, 4), (4, 5), (5, 4)):
        assert lib.ladi_op_sag_degrade(ptr(x), ptr(e), 4, ptr(m), 1, h, w, 1, 1, 0.9, 0.4, 1.0, None, ptr(o), 4, 4, stream_ptr()) != 0
        assert "5 x 5" in _lib.last_error()
    assert lib.ladi_op_sag_degrade(None, ptr(e), 4, ptr(m), 1, 5, 5, 1, 1, 0.9, 0.4, 1.0, None, ptr(o), 4, 4, stream_ptr()) != 0
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ combine: statistics and step
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_cfg_stats_sag_vs_reference(lib, B, h, w, ld):
    """factor[b] of u + g (c - u) + s (u - d) against float64 over the same fp16 values: relative error <= 1e-5, the bound of
    test_cfg_stats_vs_reference; two calls are bit-equal; scale 0 is ladi_op_cfg_stats bit for bit with NaN in the d rows"""
    hw, gs, s, phi = h * w, 7.5, 0.75, 0.7
    g = torch.Generator().manual_seed(5)
    eu = torch.randn((B, hw, 4), generator=g) * 0.8 + 0.05
    ec = torch.randn((B, hw, 4), generator=g) * (torch.arange(B).view(B, 1, 1) * 0.3 + 0.6) - 0.1
    ed = eu + torch.randn((B, hw, 4), generator=g) * 2.0
    eps = torch.cat([eu, ec, ed]).half()
    ge = U.guarded(eps.reshape(3 * B * hw, 4), ld=ld)
    e64 = eps.double()
    ref = G.rescale_factor(S.combine(e64[:B], e64[B:2 * B], e64[2 * B:], gs, s), e64[B:2 * B], phi).reshape(B)
    out = torch.full((2, B + 2), -7.0, device=U.dev())
    for k in range(2):
        assert lib.ladi_op_cfg_stats_sag(_vp(ge.ptr), ld, B, hw, gs, s, phi, ptr(out[k]), stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    rel = ((got[0, :B].double() - ref) / ref).abs().max().item()
    print("cfg_stats_sag B=%d hw=%d ld=%d: max rel err %.3g" % (B, hw, ld, rel))
    assert torch.isfinite(got[0, :B]).all() and rel <= 1e-5, rel
    assert torch.equal(got[0], got[1]) and (got[:, B:] == -7.0).all()
    plain = G.rescale_factor(G.guided_eps(e64[:B], e64[B:2 * B], gs), e64[B:2 * B], phi).reshape(B)
    assert ((ref - plain) / plain).abs().max().item() > 1e-3
    U.assert_untouched(ge, "cfg_stats_sag eps")
    eps[2 * B:] = float("nan")
    gz = U.guarded(eps.reshape(3 * B * hw, 4), ld=ld)
    z = torch.full((2, B), -7.0, device=U.dev())
    assert lib.ladi_op_cfg_stats_sag(_vp(gz.ptr), ld, B, hw, gs, 0.0, phi, ptr(z[0]), stream_ptr()) == 0, _lib.last_error()
    assert lib.ladi_op_cfg_stats(_vp(gz.ptr), ld, B, hw, gs, phi, ptr(z[1]), stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.equal(z[0], z[1])


def _mirror(kind):
    import ladi_vton_amd as L
    return {"ddim": L.DDIMScheduler, "pndm": L.PNDMScheduler, "dpmpp2m": L.DPMSolverMultistepScheduler}[kind]()


def _sched_case(kind, B, h, w, cfg, s, seed=71):
    sch = _mirror(kind)
    steps = 6
    sch.set_timesteps(steps)
    n = len(sch.timesteps)
    gtab = ([7.5, 1.0, 7.5, 1.0, 0.5, 9.0, 2.0] + [3.0] * n)[:n]
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((n, (3 if cfg else 2) * B, h * w, 4), generator=g).half()
    for i in range(n):
        if cfg and not G.is_cfg(gtab[i]):
            eps[i, :B] = float("nan")                 # a cond-only evaluation never reads its uncond rows
    if s == 0.0:
        eps[:, -B:] = float("nan")                    # scale 0 never reads the degraded input's prediction
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    return sch, steps, n, gtab, eps, lat0


def _run_sag(lib, sch, steps, n, cfg, gtab, s, E, B, hw, phi, lat0):
    L_ = lat0.permute(0, 2, 3, 1).reshape(B, hw, 4).contiguous().to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    gt = (ctypes.c_float * n)(*gtab) if cfg else None
    rc = lib.ladi_op_sched_run_sag(sch.kind, steps, _vp(ac.data_ptr()), 0.0, ptr(E), 4, n, B, hw, 1 if cfg else 0, gt, s, phi, ptr(L_), None, 0,
                                   stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return L_


@pytest.mark.parametrize("cfg,phi", [(1, 0.0), (1, 0.7), (0, 0.0)])
@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", ["ddim", "pndm", "dpmpp2m"])
def test_sched_run_sag_vs_reference(lib, kind, B, h, w, cfg, phi):
    """the step kernel's combine over a random eps sequence (a guidance table with cond-only evaluations) against the scheduler mirror with
    sag_ref.combine: rel-L2 < 1e-5, the bound of test_sched_run_pag_vs_reference.  Scale 0 with NaN in the third group is
    ladi_op_sched_run_guided over the other rows, bit for bit"""
    s = 0.75
    sch, steps, n, gtab, eps, lat0 = _sched_case(kind, B, h, w, cfg, s)
    e_nchw = eps.view(n, eps.shape[1], h, w, 4).permute(0, 1, 4, 2, 3)
    ref = S.sched_reference(sch, e_nchw, cfg, gtab, s, phi, lat0)
    got = _run_sag(lib, sch, steps, n, cfg, gtab, s, eps.to(U.dev()), B, h * w, phi, lat0).cpu().view(B, h, w, 4).permute(0, 3, 1, 2)
    err = U.rel_l2(got, ref)
    print("sched_run_sag %s B=%d hw=%d cfg=%d phi=%.1f: rel-L2 %.3g" % (kind, B, h * w, cfg, phi, err))
    assert torch.isfinite(got).all() and torch.isfinite(ref).all() and err < 1e-5, err
    off = S.sched_reference(sch, e_nchw, cfg, gtab, 0.0, phi, lat0)
    assert U.rel_l2(ref, off) > 1e-3                                         # the third term is visible at the bound
    if cfg:
        sch, steps, n, gtab, eps0, lat0 = _sched_case(kind, B, h, w, cfg, 0.0)
        zero = _run_sag(lib, sch, steps, n, cfg, gtab, 0.0, eps0.to(U.dev()), B, h * w, phi, lat0)
        E2 = eps0[:, :2 * B].contiguous().to(U.dev())
        L_ = lat0.permute(0, 2, 3, 1).reshape(B, h * w, 4).contiguous().to(U.dev())
        ac = P.alphas_cumprod().contiguous()
        rc = lib.ladi_op_sched_run_guided(sch.kind, steps, _vp(ac.data_ptr()), 0.0, ptr(E2), 4, n, B, h * w, (ctypes.c_float * n)(*gtab), phi, ptr(L_),
                                          None, 0, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert torch.isfinite(zero).all() and torch.equal(zero, L_)


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481


def build():
    """tests/tiny_tryon.py build() over the peaked checkpoint (sag_ref.peaked)"""
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=S.peaked(C.synth_state_dict(C.unet_shapes(ucfg), "unet.")), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, fwd={}, inp={})


@pytest.fixture(scope="module")
def tiny():
    t = build()
    yield t
    t["mod"]["unet"].set_sag_capture(False)
    t["mod"]["unet"].disable_freeu()


@pytest.mark.parametrize("hw", [(64, 48), (52, 38)])
def test_forward_map_vs_reference(tiny, hw):
    """NativeUNet tiny (peaked), n = 2 different samples, t = 481, capture on: the library's (s, m) against sag_ref's float32 forward.  The
    band is twice the largest difference between the reference in float32 and the reference with checkpoint and activations in fp16 on the
    CPU (measured: 0.019 at 64x48 and 0.020 at 52x38 on the GPU host, whose largest |s - s_ref| were 0.011 and 0.016; 0.039 and 0.022 on a
    host with other fp16 CPU kernels): s is within the band everywhere, m is exact outside it, at most 15 % of the tokens
    lie inside it, and the forward's output is bit-equal to the forward without capture"""
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = TT.unet_inputs(tiny, hw, n=2)
    s_ref, band = S.band_of(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs)
    hm, wm = S.map_size(*hw)
    assert unet.sag_tokens(*hw) == (hm, wm)
    unet.set_sag_capture(False)
    plain = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    unet.set_sag_capture(True)
    on = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    s, m = unet.sag_map()
    s, m = s.cpu().reshape(2, hm * wm), m.cpu().reshape(2, hm * wm)
    unet.set_sag_capture(False)
    assert torch.equal(on, plain)
    err = float((s - s_ref).abs().max())
    inside = (s_ref - 1.0).abs() <= band
    print("SAG map %dx%d: T = %d, band %.4g, max |s - s_ref| %.4g, inside the band %.3f, ones %.2f" % (hw + (hm * wm, band, err, float(inside.float().mean()),
                                                                                                        float(m.float().mean()))))
    U.record_parity("sag_map_tiny_%dx%d" % hw, dict(band=band, max_err=err, inside=float(inside.float().mean())))
    assert torch.isfinite(s).all() and err <= band, (err, band)
    assert torch.equal(m[~inside], S.mask_of(s_ref)[~inside])
    assert float(inside.float().mean()) <= 0.15
    assert torch.equal(m, S.mask_of(s))
    # the rows form: sample 1 alone, at its own row of the buffers; sample 0's row stays
    unet.set_sag_capture(True)
    unet(xd[1:].contiguous(), T0, encoder_hidden_states=ed, sample0=1)
    s2, m2 = unet.sag_map(n=2, latent_size=hw)
    unet.set_sag_capture(False)
    s2, m2 = s2.cpu().reshape(2, -1), m2.cpu().reshape(2, -1)
    assert torch.equal(s2[0], s[0]) and torch.equal(m2[0], m[0])
    # a forward of one sample may select other tiles than the forward of two (fp16 rounding of another summation order): the band again
    assert float((s2[1] - s_ref[1]).abs().max()) <= band and torch.equal(m2[1], S.mask_of(s2[1]))


def test_map_misuse(tiny, lib):
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = TT.unet_inputs(tiny, (64, 48), n=2)
    unet.set_sag_capture(True)
    unet(xd, T0, encoder_hidden_states=ed)
    unet.set_sag_capture(False)
    with pytest.raises(_lib.NativeError, match="48 tokens"):
        unet.sag_map(n=2, latent_size=(52, 38))
    with pytest.raises(_lib.NativeError, match="room for"):
        unet.sag_map(n=64, latent_size=(64, 48))
    assert lib.ladi_unet_set_sag_capture(None, 1) == -1 and lib.ladi_tryon_set_sag(None, 0.5) == -1


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
SAG = 0.75
BIG, SMALL = (512, 384), (256, 192)               # latents 64 x 48 (the map has 48 tokens) and 32 x 24 (12 tokens)
CASES = {
    "plain": dict(sag_scale=0.0, steps=6),
    "base": dict(steps=6),
    "pndm": dict(scheduler="pndm", steps=5),
    "nocfg": dict(guidance=1.0, steps=6),
    "cutoff": dict(table=[7.5, 7.5, 1.0, 7.5, 7.5, 7.5], steps=6),
    "rescale": dict(phi=0.7, steps=3, size=SMALL),
    "freeu": dict(freeu=(0.9, 0.2, 1.4, 1.6), steps=3, size=SMALL),
    "strength": dict(steps=4, size=SMALL, strength=0.75, preserve=("both", 0.0)),
}


def _masks_callback(pipe, case, arm, store):
    """the step callback that reads the base group's mask of evaluation i back (the first forward's: the second does not capture)"""
    kw = CASES[case]
    H, W = kw.get("size", BIG)
    table = kw.get("table")
    cfg = any(g > 1.0 for g in table) if table else kw.get("guidance", 7.5) > 1.0

    def cb(i, t, lat):
        cond_only = cfg and table is not None and not table[i] > 1.0
        n = 4 if cfg and arm != "modular" else 2
        s, m = pipe.unet.sag_map(n=n, latent_size=(H // 8, W // 8))
        r0 = 2 if (cond_only and arm != "modular") else 0
        store.append(m[r0:r0 + 2].cpu().clone())
    return cb


def _pipe_args(tiny, case):
    kw = CASES[case]
    args = dict(guidance_scale=kw.get("table", kw.get("guidance", 7.5)), guidance_rescale=kw.get("phi", 0.0), sag_scale=kw.get("sag_scale", SAG),
                num_inference_steps=kw["steps"])
    if "strength" in kw:
        args.update(strength=kw["strength"], init_latents=_init(tiny, kw), preserve_unmasked=kw["preserve"][0])
    return args


def _init(tiny, kw):
    H, W = kw.get("size", BIG)
    return torch.randn((2, 4, H // 8, W // 8), generator=torch.Generator().manual_seed(77))


def _run(tiny, case, arm):
    """one run per (case, arm) on a fresh pipeline -> (images, latents, masks per evaluation)"""
    if (case, arm) not in tiny["run"]:
        kw = CASES[case]
        pipe = TT.pipe(tiny, kw.get("scheduler", "ddim"))
        pipe.enable_freeu(*kw["freeu"]) if kw.get("freeu") else pipe.disable_freeu()
        masks = []
        cb = _masks_callback(pipe, case, arm, masks) if kw.get("sag_scale", SAG) > 0 else None
        fused, graph = TT.ARMS[arm]
        img, lat = TT.call(tiny, pipe, TT.inputs(tiny, 2, *kw.get("size", BIG)), fused, graph, callback=cb, **_pipe_args(tiny, case))
        pipe.disable_freeu()
        tiny["run"][(case, arm)] = (img, lat, masks, pipe)
    return tiny["run"][(case, arm)]


def _ref(tiny, case, masks):
    if case not in tiny["ref"]:
        kw = CASES[case]
        extra = {}
        if "strength" in kw:
            first = kw["steps"] - min(int(kw["steps"] * kw["strength"]), kw["steps"])
            extra = dict(init_latents=_init(tiny, kw), first_step=first, preserve=kw["preserve"])
        info = {}
        img, lat = S.tryon_sag_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"],
                                         TT.inputs(tiny, 2, *kw.get("size", BIG)), kw["steps"], kw.get("scheduler", "ddim"),
                                         sag_scale=kw.get("sag_scale", SAG), guidance=kw.get("guidance", 7.5), table=kw.get("table"), phi=kw.get("phi", 0.0),
                                         freeu=kw.get("freeu"), forced_masks=masks or None, info=info, **extra)
        tiny["ref"][case] = (img, lat, info)
    return tiny["ref"][case]


@pytest.mark.parametrize("case", ["base", "pndm", "nocfg", "cutoff"])
def test_loop_vs_reference(tiny, case):
    """B = 2, latents 64 x 48: DDIM with 6 steps and PNDM with 5, with CFG, without, and with one cond-only evaluation in a guidance
    schedule, sag_scale 0.75, against tryon_sag_reference with the masks the fused run read back per evaluation forced (the UNet-level test
    pins the mask itself).  Thresholds of tests/test_gpu_pag.py's end-to-end case: latents >= 40 dB, image >= 35 dB.  Graph replay is
    bit-equal to eager launches, and the modular path meets the same reference"""
    img, lat, masks, pipe = _run(tiny, case, "graph")
    evals = CASES[case]["steps"] + (1 if case == "pndm" else 0)
    assert len(masks) == evals and all(m.shape == (2, 8, 6) for m in masks)
    ones = [float(m.float().mean()) for m in masks]
    print("SAG %s: share of ones per evaluation %s" % (case, ["%.2f" % o for o in ones]))
    assert all(0.05 <= o <= 0.95 for o in ones), ones
    ref_img, ref_lat, info = _ref(tiny, case, masks)
    p_img, p_lat = TT.assert_close("tiny SAG %s graph" % case, img, lat, ref_img, ref_lat)
    U.record_parity("sag_tiny_%s_graph" % case, dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    agree = [float((m == S.mask_of(s)).float().mean()) for m, s in zip(masks, info["sums"])]
    print("SAG %s: device masks agree with the reference's own on %s of the tokens" % (case, ["%.2f" % a for a in agree]))
    if case == "cutoff":
        assert info["cond_only"] == 1 and pipe.cond_only_evals() == 1
    if case == "nocfg":
        assert info["cond_only"] == evals
    img_e, lat_e, masks_e, _ = _run(tiny, case, "eager")
    assert torch.equal(lat, lat_e) and torch.equal(img, img_e) and all(torch.equal(a, b) for a, b in zip(masks, masks_e))
    if case in ("base", "cutoff"):
        img_m, lat_m, masks_m, _ = _run(tiny, case, "modular")
        TT.assert_close("tiny SAG %s modular" % case, img_m, lat_m, ref_img, ref_lat)
        p = U.psnr(lat_m, lat)
        print("SAG %s fused against modular: latents %.2f dB" % (case, p))
        assert p >= 40.0, p
    if case == "base":
        plain_img, plain_lat, _, _ = _run(tiny, "plain", "graph")
        assert U.psnr(lat, plain_lat) < 40.0                             # and it is not the plain loop


def test_no_stale_graph_and_scale_from_device_memory(tiny, lib):
    """one pipeline with use_graph: plain -> SAG 0.75 -> SAG 0.3 -> sag_scale = 0.  The first and the last run are bit-equal (and equal a fresh
    plain run); the two SAG runs differ, the second without a new capture (the graph table is the first's: its executables keep their
    addresses), and a fresh pipeline at 0.3 gives the second run's bits"""
    inp = TT.inputs(tiny, 2, *SMALL)
    call = lambda p, s: TT.call(tiny, p, inp, True, True, num_inference_steps=4, sag_scale=s)
    pipe = TT.pipe(tiny)
    img_1, lat_1 = call(pipe, 0.0)
    img_2, lat_2 = call(pipe, 0.75)
    caps = lib.ladi_tryon_graph_captures(pipe._tryon)
    img_3, lat_3 = call(pipe, 0.3)
    assert lib.ladi_tryon_graph_captures(pipe._tryon) == caps and caps >= 2          # another scale replays the graphs of the first
    img_4, lat_4 = call(pipe, 0.0)
    assert lib.ladi_tryon_graph_captures(pipe._tryon) > caps                          # switching SAG off is another key
    assert torch.equal(lat_4, lat_1) and torch.equal(img_4, img_1)
    assert U.psnr(lat_2, lat_3) < 60.0 and U.psnr(lat_2, lat_1) < 40.0
    fresh = TT.pipe(tiny)
    img_5, lat_5 = call(fresh, 0.3)
    assert torch.equal(lat_5, lat_3) and torch.equal(img_5, img_3)
    img_6, lat_6 = call(TT.pipe(tiny), 0.0)
    assert torch.equal(lat_6, lat_1)


def test_lanes(tiny):
    """two sample-group lanes (the second forward runs its two samples on two lanes too) against one: latents >= 45 dB"""
    inp = TT.inputs(tiny, 2, *SMALL)
    one = TT.pipe(tiny)
    _, lat_1 = TT.call(tiny, one, inp, True, True, num_inference_steps=4, sag_scale=SAG)
    two = TT.pipe(tiny)
    two.lanes = 2
    _, lat_2 = TT.call(tiny, two, inp, True, True, num_inference_steps=4, sag_scale=SAG)
    assert two.lib_lanes() == 2
    p = U.psnr(lat_2, lat_1)
    print("SAG two lanes against one: latents %.2f dB" % p)
    assert p >= 45.0, p


def test_refusals_leave_the_handle_usable(tiny, lib):
    """every refusal raises before anything is launched, and the next plain run on the same handle is the plain run"""
    import ladi_vton_amd as L
    inp, d = TT.inputs(tiny, 2, *SMALL), U.dev()
    pipe = TT.pipe(tiny)
    call = lambda p=pipe, **kw: TT.call(tiny, p, inp, True, True, num_inference_steps=4, **kw)
    img_1, lat_1 = call()
    with pytest.raises(ValueError, match="feature_cache"):
        call(sag_scale=SAG, feature_cache=2)
    with pytest.raises(ValueError, match="pag_scale"):
        call(sag_scale=SAG, pag_scale=3.0)
    with pytest.raises(ValueError, match="sag_scale"):
        call(sag_scale=-1.0)
    for cls in (L.EulerDiscreteScheduler, L.EulerAncestralDiscreteScheduler, L.LMSDiscreteScheduler):
        with pytest.raises(ValueError, match=cls.__name__):
            TT.call(tiny, L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                                          scheduler=cls(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5]),
                    inp, True, True, num_inference_steps=4, sag_scale=SAG)
    small = TT.inputs(tiny, 2, 32, 32)
    with pytest.raises(ValueError, match="5 x 5"):
        TT.call(tiny, pipe, small, True, True, num_inference_steps=4, sag_scale=SAG)
    # the native refusals behind the Python checks, through the fused entry itself
    a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
         inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], SMALL[0], SMALL[1], 4, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="feature-cache plan"):
        pipe._run_fused(*a, sag_scale=SAG, feature_cache=([1, 0, 1, 0], 0))
    with pytest.raises(_lib.NativeError, match="positive PAG scale"):
        pipe._run_fused(*a, sag_scale=SAG, pag_table=[3.0] * 4)
    euler = TT.pipe(tiny, "euler")
    euler._run_fused(*a)
    with pytest.raises(_lib.NativeError, match="sigma-space"):
        euler._run_fused(*a, sag_scale=SAG)
    b = (small["image"], small["mask_image"].clone(), small["pose_map"], small["warped_cloth"], small["prompt_embeds"].to(d),
         small["negative_prompt_embeds"].to(d), small["noise_cloth"], small["noise_latents"], small["noise_masked"], 32, 32, 4, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="5 x 5"):
        pipe._run_fused(*b, sag_scale=SAG)
    assert lib.ladi_tryon_set_sag(pipe._tryon, -1.0) == -1 and lib.ladi_tryon_set_sag(pipe._tryon, float("nan")) == -1
    img_2, lat_2 = call()
    assert torch.equal(lat_2, lat_1) and torch.equal(img_2, img_1)
    img_3, lat_3 = call(sag_scale=SAG)
    assert torch.isfinite(lat_3).all() and U.psnr(lat_3, lat_1) < 40.0


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("case", ["rescale", "freeu", "strength"])
def test_composition_vs_reference(tiny, case):
    """one short SAG run (latents 32 x 24) with guidance rescale, with FreeU, and with strength < 1 plus preserve_unmasked = "both": against
    the reference with the device's masks forced, the end-to-end thresholds; graph replay bit-equal to eager"""
    img, lat, masks, _ = _run(tiny, case, "graph")
    ref_img, ref_lat, _ = _ref(tiny, case, masks)
    TT.assert_close("tiny SAG %s graph" % case, img, lat, ref_img, ref_lat)
    img_e, lat_e, _, _ = _run(tiny, case, "eager")
    assert torch.equal(lat, lat_e) and torch.equal(img, img_e)


def _fused_vs_modular(tiny, what, pipe, **kw):
    inp = TT.inputs(tiny, 2, *SMALL)
    img_f, lat_f = TT.call(tiny, pipe, inp, True, True, num_inference_steps=3, sag_scale=SAG, **kw)
    img_m, lat_m = TT.call(tiny, pipe, inp, False, False, num_inference_steps=3, sag_scale=SAG, **kw)
    img_p, lat_p = TT.call(tiny, pipe, inp, True, True, num_inference_steps=3, **kw)
    p, q = U.psnr(lat_f, lat_m), U.psnr(lat_f, lat_p)
    print("SAG with %s: fused against modular %.2f dB, against the run without SAG %.2f dB" % (what, p, q))
    assert torch.isfinite(lat_f).all() and p >= 40.0 and q < 40.0, (p, q)


def test_composition_ip_adapter(tiny):
    """an image prompt: the second forward reads the base group's image tokens; against the reference with the masks forced"""
    unet, E = tiny["mod"]["unet"], 64
    sd_ip = IPR.make_adapter(tiny["ucfg"], 4, E)
    unet.load_ip_adapter(IPR.to_diffusers(sd_ip, 2, numbered=True))
    try:
        emb = torch.randn((2, E), generator=torch.Generator().manual_seed(9)).half().float()
        pipe = TT.pipe(tiny)
        pipe.set_ip_adapter_scale(1.0)
        masks = []
        CASES["_ip"] = dict(steps=3, size=SMALL)
        inp = TT.inputs(tiny, 2, *SMALL)
        img, lat = TT.call(tiny, pipe, inp, True, True, num_inference_steps=3, sag_scale=SAG, ip_adapter_image_embeds=emb.to(U.dev()),
                           callback=_masks_callback(pipe, "_ip", "graph", masks))
        ref_img, ref_lat = S.tryon_sag_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp, 3, "ddim",
                                                 sag_scale=SAG, ip=(sd_ip, emb, None, [1.0] * 16), forced_masks=masks)
        TT.assert_close("tiny SAG with an image prompt", img, lat, ref_img, ref_lat)
    finally:
        CASES.pop("_ip", None)
        unet.unload_ip_adapter()


def test_composition_lora_and_token_merging(tiny):
    """a LoRA adapter, then token merging at max_downsample = 1 (the mid block does not merge): fused against modular for a seed"""
    unet = tiny["mod"]["unet"]
    b = "down_blocks.0.attentions.0.transformer_blocks.0"
    shapes = {b + ".attn1.to_q": (64, 64), "mid_block.attentions.0.transformer_blocks.0.attn1.to_k": (256, 256)}
    unet.load_lora_adapter(LR.make_adapter(3, shapes, {m: 4 for m in shapes}), "sag")
    try:
        unet.set_adapters(["sag"], [1.0])
        _fused_vs_modular(tiny, "a LoRA adapter", TT.pipe(tiny))
    finally:
        unet.set_adapters([])
        unet.delete_adapters(["sag"])
    pipe = TT.pipe(tiny)
    pipe.apply_token_merging(ratio=0.5, max_downsample=1)
    try:
        _fused_vs_modular(tiny, "token merging", pipe)
    finally:
        pipe.remove_token_merging()
