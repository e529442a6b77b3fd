"""Kernels on operands past the 2 GiB and 4 GiB byte offsets, judged element by element (tests/far_cases.py has the why and the builders).

Every case is a correct program -- strides only -- judged like tests/test_gpu_views.py: float64 reference, the operator's *_ref_bound,
check_elem per element, the poison of every operand and of the output counted on the device (tests/util.py assert_untouched_far), the worst
err / limit recorded under "far/..." keys.  A case either passes or is cleanly refused by the host (non-zero rc, a ladi_last_error text,
nothing written); every implicit-GEMM case asserts the family that ran.  Each test holds less than 10 GiB on the device and returns it.

    (a) rebasing works       samples of a multiple of the tile's pixels, about 1.25 GiB each, the tensor beyond 2^32 bytes
    (b) a tile straddles     64-pixel samples under 128- / 256-pixel tiles, the second sample of a tile past 0x7FFFFFFF, the third past 2^32:
                             right or refused (rc -20), never NaN or zero-fed; and the largest stride the span guard accepts, found on the host
    (c) the other operands   out, res0, res1 far in turn (mask and the fused statistics rows have no stride: they ride along)
    (d) halo and linear_xs   just below their byte limit: taken and right; one stride step above: refused, cfg 0 runs another family"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from tests import far_cases as FC
from tests import stats_cases as S
from tests import util as U

pytestmark = pytest.mark.gpu
GIB = 1 << 30


def _rec(test, case, ratio, offset):
    U.record_parity("far/%s[%s]" % (test, case), dict(ratio=round(ratio, 4), largest_byte_offset=int(offset)))


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class _cost_model:
    """cfg 0 launches inside choose by the cost model (deterministic), not by timing every configuration"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.lib.ladi_igemm_set_autotune(0)

    def __exit__(self, *exc):
        self.lib.ladi_igemm_set_autotune(1)


@functools.lru_cache(maxsize=None)
def _conv(form, N, h, w, **kw):
    return FC.FarConv(N=N, h=h, w=w, **dict(FC.FORMS[form], **kw))


def _cfgs_for(lib, pb, batch=1):
    """the tiled configurations of far_cases.TILED that take problem pb at ordinary strides, and 0"""
    d = pb.desc()
    return [c for cfgs in FC.TILED.values() for c in cfgs if FC.admissible(lib, d, c, batch)] + [0]


def _run_right(lib, pl, cfg, test, case, family=None):
    """a launch that has to be accepted and right; records it; returns the launch info"""
    rc, out, _ = pl.launch(lib, cfg)
    assert rc == 0, "%s %s cfg %d refused: rc = %d (%s)" % (test, case, cfg, rc, _lib.last_error())
    info = FC.last_launch(lib)
    sel = FC.last_selection(lib)[0]
    what = "%s %s cfg %d -> %d %s" % (test, case, cfg, sel, info)
    ratio = pl.check(out, what)
    want = family or (FC.family_of(cfg) if cfg else None)
    if want:
        assert info["family"] == want, what
    else:
        assert info["family"] == FC.family_of(sel), what
    _rec(test, "%s-cfg%d" % (case, cfg), ratio, pl.largest_offset())
    del out
    return info, sel


def _run_right_or_refused(lib, pl, cfg, test, case):
    """(b): right, or refused with a non-zero rc and an error text and nothing written; returns the rc"""
    rc, out, _ = pl.launch(lib, cfg)
    if rc != 0:
        text = _lib.last_error()
        assert text and str(rc) in text, (test, case, cfg, rc, text)
        FC.assert_nothing_written(out, "%s %s cfg %d rc %d" % (test, case, cfg, rc))
        pl.check_inputs("%s %s cfg %d rc %d" % (test, case, cfg, rc))
        assert FC.last_launch(lib)["family"] == 0 or rc in (-20,), (test, case, cfg, rc)
        U.record_parity("far/%s[%s-cfg%d]" % (test, case, cfg), dict(refused=rc, largest_byte_offset=int(pl.largest_offset())))
        return rc
    info = FC.last_launch(lib)
    sel = FC.last_selection(lib)[0]
    what = "%s %s cfg %d -> %d %s" % (test, case, cfg, sel, info)
    ratio = pl.check(out, what)
    assert info["family"] == FC.family_of(sel), what
    _rec(test, "%s-cfg%d" % (case, cfg), ratio, pl.largest_offset())
    return 0


# ---------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("form,far", [("conv3x3", "src0"), ("conv3x3_s2", "src0"), ("conv1x1", "src0"), ("ups", "src0"), ("two_src", "src0"), ("two_src", "src1")])
def test_igemm_rebased_tiles_reach_past_4_gib(lib, form, far):
    """four samples whose OUTPUT has 256 pixels (every 64- / 128- / 256-pixel tile lies inside one sample), the far source at a row stride that
    makes a sample 1.25 GiB: sample 1 crosses the 2 GiB mark, samples 3 starts past 4 GiB, yet every tile stays under 2^31 bytes from its
    rebased base.  Small and large tiles of the ring, igemm8 and loader / consumer families, and cfg 0."""
    hw = dict(conv3x3_s2=(32, 32), ups=(8, 8)).get(form, (16, 16))
    pb = _conv(form, 4, *hw)
    assert pb.Ho * pb.Wo == 256
    ld = FC.ld_for_bytes(pb.h * pb.w + 1, 5 * GIB // 4)
    pl = None
    try:
        pl = pb.place({far: ld})
        assert pl.g[far].last_byte > FC.MARK32 and pl.g[far].bytes < 6 * GIB
        with _cost_model(lib):
            for cfg in _cfgs_for(lib, pb):
                assert FC.admissible(lib, pb.desc({far: ld}), cfg) or cfg == 0, (form, far, cfg)
                _run_right(lib, pl, cfg, "igemm_rebased", "%s-%s" % (form, far))
    finally:
        if pl is not None:
            pl.close()
        del pl
        _release()


def test_igemm_batched_launch_with_batch_strides_past_4_gib(lib):
    """batch = 2 problems of [256, 64] x [64, 64]^T whose elements lie 2^31 + 64 halves (4 GiB + 128 B) apart: bs_src0 and bs_out in one
    launch, bs_res and bs_out in the next (three such operands at once would pass 10 GiB).  The batch stride is added with 64 bits."""
    B, P, K, Q, bs = 2, 256, 64, 64, (1 << 31) + 64
    x, w, r = [FC.rand((P, K), 940 + b) for b in range(B)], FC.rand((Q, K), 950, 0.125), [FC.rand((P, Q), 960 + b) for b in range(B)]
    ref, bound = U.gemm_batched_ref_bound(x, [w], res=r)
    W = w.half().to(U.dev())
    for far in (("src0", "out"), ("res", "out")):
        X = R = out = None
        try:
            X = U.guarded_far(torch.cat(x).half(), K + 64, samples=B, sstride=bs if "src0" in far else P * (K + 64) + 64)
            R = U.guarded_far(torch.cat(r).half(), Q + 64, samples=B, sstride=bs if "res" in far else P * (Q + 64) + 64)
            for cfg in (9, 20, 56, 0):
                out = U.guarded_far_out(B * P, Q, Q + 8, samples=B, sstride=bs)
                d = _lib.IGemmDesc()
                d.src0, d.C0, d.ld0, d.bs_src0 = X.ptr, K, X.ld, X.sstride
                d.Hs, d.Ws, d.Ho, d.Wo, d.P, d.ksize, d.stride = P, 1, P, 1, P, 1, 1
                d.W, d.Q, d.K, d.out_scale = W.data_ptr(), Q, K, 1.0
                d.res0, d.ldr0, d.bs_res = R.ptr, R.ld, R.sstride
                d.out, d.ldo, d.bs_out = out.ptr, out.ld, out.sstride
                with _cost_model(lib):
                    rc = lib.ladi_op_igemm(ctypes.byref(d), B, cfg, stream_ptr())
                torch.cuda.synchronize()
                assert rc == 0, (far, cfg, rc, _lib.last_error())
                info, what = FC.last_launch(lib), "igemm_batched %s cfg %d" % ("+".join(far), cfg)
                assert info["family"] == (FC.family_of(cfg) if cfg else FC.family_of(FC.last_selection(lib)[0])), (what, info)
                ratio = U.check_elem(out.cpu().float(), ref.reshape(B * P, Q), bound.reshape(B * P, Q), what)
                for g, name in ((out, "output"), (X, "x"), (R, "res")):
                    U.assert_untouched_far(g, what + " " + name)
                _rec("igemm_batched", "%s-cfg%d" % ("+".join(far), cfg), ratio, max(out.last_byte, X.last_byte, R.last_byte))
                out = None
        finally:
            del X, R, out
            _release()


# ---------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("form", ["conv3x3", "conv1x1"])
def test_igemm_tile_straddling_samples_is_right_or_refused(lib, form):
    """three samples of 8 x 8 pixels at a row stride of 2^24 + 8 halves: sample 1 starts past 0x7FFFFFFF, sample 2 past 2^32.  A 128-pixel tile
    holds two samples, a 256-pixel tile all three; every gather of the second sample lies outside a descriptor of 0x7FFFFFFF bytes that
    starts at the first.  Each launch is right or refused -- never NaN, never zero-fed.  With the span guard (rc -20) every straddling tile
    is refused; the 1 x 1 form still runs on 64-pixel tiles (one sample each: 63 rows = 2.11e9 bytes, under the limit), and cfg 0 has to find
    them; the 3 x 3 form (pad rows and pixels: 72 rows) is out of reach of every tile and refused as a whole.
    Measured with the guard taken out: rc 0 everywhere; the 128-pixel tiles return sample 1 exactly as if x were zero (64 of 64 pixels equal
    to bias + residual), the 256-pixel tiles that and NaN for all of sample 2 (the offset wraps past 2^32 into poison), and the 3 x 3 form on
    64-pixel tiles misses the bound in about 1150 of 4096 elements of every sample."""
    pb = _conv(form, 3, 8, 8)
    ld = (1 << 24) + 8
    pl = None
    try:
        pl = pb.place(dict(src0=ld))
        assert pl.g["src0"].last_byte > FC.MARK32 and 64 * ld * 2 > FC.LIMIT
        rcs = {}
        with _cost_model(lib):
            for cfg in _cfgs_for(lib, pb):
                rcs[cfg] = _run_right_or_refused(lib, pl, cfg, "igemm_straddle", form)
        if form == "conv1x1":
            assert rcs[0] == 0 and rcs[9] == 0 and rcs[66] == 0, rcs
            assert FC.bp_of(FC.last_selection(lib)[0]) == 64
        d = pb.desc(dict(src0=ld))
        for cfg, rc in rcs.items():
            if cfg:
                assert (rc == 0) == FC.admissible(lib, d, cfg), (cfg, rc)           # the launch and the host-only rule agree
    finally:
        if pl is not None:
            pl.close()
        del pl
        _release()


@pytest.mark.parametrize("cfg", [20, 56, 62, 19])
def test_igemm_largest_stride_the_span_guard_accepts(lib, cfg):
    """the boundary, in two steps: the host finds the largest ld0 at which the guard admits a straddling launch (3 x 3 over three 64-pixel
    samples; the 128-pixel tiles of cfg 20 / 56 / 62 hold two samples, the 256-pixel tile of cfg 19 all three), then exactly that launch
    runs.  Its last gathers end within 16 ld bytes of 0x7FFFFFFF from the tile's base: a guard that is too lenient fails here."""
    pb = _conv("conv3x3", 3, 8, 8)
    d = pb.desc()
    ld = FC.largest_admissible(lib, d, "ld0", cfg, 128, 1 << 30)
    span = FC.tile_span(d, FC.bp_of(cfg))[0]
    assert FC.LIMIT - 2 * 8 * (2 * 64 + 72) <= span < FC.LIMIT, (cfg, ld, span)
    pl = None
    try:
        pl = pb.place(dict(src0=ld))
        _run_right(lib, pl, cfg, "igemm_span_boundary", "ld%d" % ld)
    finally:
        if pl is not None:
            pl.close()
        del pl
        _release()


# ---------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("far", ["out", "res0", "res1"])
def test_igemm_far_output_and_residuals(lib, far):
    """the source near, out / res0 / res1 far in turn (256 rows at a stride that puts the last one past 2^32 bytes, the middle past 2^31), with
    SiLU, both residuals, the mask and the fused statistics rows: every family's epilogue (fast rows, split-K combine, halo), and cfg 0.
    The statistics rows a launch reports are judged against the output it stored (tests/stats_cases.py judge_rows)."""
    pb = _conv("conv3x3", 4, 8, 8, act="silu", res1=True, mask=True, seed=920)
    ld = FC.ld_for_bytes(pb.P, FC.MARK32)
    pl = None
    try:
        pl = pb.place({far: ld})
        with _cost_model(lib):
            extra = [c for c in (FC.SPLIT_K, FC.HALO[0]) if FC.admissible(lib, pb.desc(), c)]
            assert len(extra) == 2
            for cfg in _cfgs_for(lib, pb)[:-1] + extra + [0]:
                st = S.poisoned_rows(pb.P, pb.cout)
                rc, out, px = pl.launch(lib, cfg, stats=st)
                assert rc == 0, (far, cfg, rc, _lib.last_error())
                info, sel = FC.last_launch(lib), FC.last_selection(lib)[0]
                what = "igemm_far_epilogue %s cfg %d -> %d %s" % (far, cfg, sel, info)
                assert info["family"] == FC.family_of(sel) and (cfg == 0 or sel == cfg), what
                if cfg == FC.SPLIT_K:
                    assert info["split"] == 2, what
                ratio = pl.check(out, what)
                if px:
                    ratio = max(ratio, S.judge_rows(st, px, out.cpu().double(), pb.N, pb.Ho * pb.Wo, what + " px %d" % px))
                else:
                    S.assert_all_poison(st, what + " (reported px = 0)")
                _rec("igemm_far_epilogue", "%s-cfg%d" % (far, cfg), ratio, pl.largest_offset())
                del out, st
    finally:
        if pl is not None:
            pl.close()
        del pl
        _release()


# ---------------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("cfg", FC.HALO)
def test_halo_below_and_above_its_byte_limit(lib, cfg):
    """four 8 x 8 samples: at the largest ld0 with P ld0 2 < 0x7FFFFFFF the halo form is taken and right; one stride step above it is refused
    (rc -16, nothing written) and cfg 0 runs the launch on another family, right."""
    pb = _conv("conv3x3", 4, 8, 8)
    d = pb.desc()
    ld = FC.largest_admissible(lib, d, "ld0", cfg, 128, 1 << 30)
    assert pb.P * ld * 2 < FC.LIMIT <= pb.P * (ld + 8) * 2
    for step, stride in (("below", ld), ("above", ld + 8)):
        pl = None
        try:
            pl = pb.place(dict(src0=stride))
            if step == "below":
                _run_right(lib, pl, cfg, "halo_limit", "below", family="halo")
            else:
                rc, out, _ = pl.launch(lib, cfg)
                assert rc != 0 and _lib.last_error(), rc
                FC.assert_nothing_written(out, "halo_limit above cfg %d" % cfg)
                del out
                with _cost_model(lib):
                    info, sel = _run_right(lib, pl, 0, "halo_limit", "above-after-cfg%d" % cfg)
                assert info["family"] != "halo", (info, sel)
        finally:
            if pl is not None:
                pl.close()
            del pl
            _release()


def test_linear_xs_below_and_above_its_residual_limit_and_far_x(lib):
    """the X-stationary residual form (cfg 25) on 128 tokens, K = Q = 320: at the largest ldr0 with P ldr0 2 < 0x7FFFFFFF it is taken and right, one
    step above it is refused and cfg 0 runs another family, right; and with x itself at a row stride that puts its last row past 2^32 bytes (beyond any tiled
    kernel's reach, rc -20 for them) the kernel's 64-bit pixel addressing is right, for cfg 25 and for cfg 0, which must find it."""
    pb = FC.FarConv(N=1, h=128, w=1, c0=320, cout=320, ksize=1, pad=0, seed=930)
    d = pb.desc()
    ldr = FC.largest_admissible(lib, d, "ldr0", 25, 384, 1 << 30)
    assert pb.P * ldr * 2 < FC.LIMIT <= pb.P * (ldr + 8) * 2
    for case, ld in (("res-below", dict(res0=ldr)), ("res-above", dict(res0=ldr + 8)), ("x-far", dict(src0=FC.ld_for_bytes(pb.P, FC.MARK32)))):
        pl = None
        try:
            pl = pb.place(ld)
            with _cost_model(lib):
                if case == "res-above":
                    rc, out, _ = pl.launch(lib, 25)
                    assert rc != 0 and _lib.last_error(), rc
                    FC.assert_nothing_written(out, "linear_xs_limit above")
                    del out
                    info, _ = _run_right(lib, pl, 0, "linear_xs_limit", case)
                    assert info["family"] != "linear_xs", info
                else:
                    _run_right(lib, pl, 25, "linear_xs_limit", case, family="linear_xs")
                    if case == "x-far":
                        assert pl.g["src0"].last_byte > FC.MARK32
                        rc, out, _ = pl.launch(lib, 9)
                        assert rc == -20 and "span" in _lib.last_error() and "HsWs" in _lib.last_error(), (rc, _lib.last_error())
                        FC.assert_nothing_written(out, "linear_xs_limit x-far cfg 9")
                        del out
                        info, _ = _run_right(lib, pl, 0, "linear_xs_limit", case + "-cfg0", family="linear_xs")
        finally:
            if pl is not None:
                pl.close()
            del pl
            _release()


# ---------------------------------------------------------------------------------------------------------------------- other operators
def _far_pair(rows):
    """two strides for `rows` rows: the last row past 2^31 bytes / past 2^32 bytes"""
    return FC.ld_for_bytes(rows, FC.MARK31), FC.ld_for_bytes(rows, FC.MARK32)


def test_layer_norm_far_rows(lib):
    """ladi_op_layer_norm_ld on 77 rows of 512: x at a stride that puts the last row past 2^32 bytes, out past 2^31, then the other way round"""
    rows, C = 77, 512
    x, g, b = FC.rand((rows, C), 36, 3.0) + 1, FC.rand((C,), 37, 0.1) + 1, FC.rand((C,), 38, 0.1)
    x, g = x.half().float(), g.half().float()
    ref, bound = U.layer_norm_ref_bound(x, g, b, 1e-5)
    G, B = g.half().to(U.dev()), b.half().to(U.dev())
    l31, l32 = _far_pair(rows)
    for case, ldx, ldo in (("x32-o31", l32, l31), ("x31-o32", l31, l32)):
        X = out = None
        try:
            X, out = U.guarded_far(x.half(), ldx), U.guarded_far_out(rows, C, ldo)
            assert lib.ladi_op_layer_norm_ld(X.ptr, X.ld, ptr(G), ptr(B), 1e-5, rows, C, out.ptr, out.ld, stream_ptr()) == 0, _lib.last_error()
            torch.cuda.synchronize()
            what = "layer_norm_far " + case
            ratio = U.check_elem(out.cpu().float(), ref, bound, what)
            U.assert_untouched_far(out, what + " output")
            U.assert_untouched_far(X, what + " input")
            _rec("layer_norm", case, ratio, max(X.last_byte, out.last_byte))
        finally:
            del X, out
            _release()


def _heads(t, n, heads, hd):
    return t.reshape(n, -1, heads, hd).transpose(1, 2)


ATTN = dict(flash=(2, 2, 64, 192, 192), flash_qb2=(4, 10, 64, 2600, 300), causal=(2, 2, 64, 77, 77), generic=(2, 2, 80, 257, 257))


@functools.lru_cache(maxsize=None)
def _attn_ref(kind):
    n, heads, hd, Nq, Nk = ATTN[kind]
    C = heads * hd
    q, k, v = FC.rand((n, Nq, C), 230), FC.rand((n, Nk, C), 231), FC.rand((n, Nk, C), 232)
    ref, bound = U.attention_ref_bound(_heads(q, n, heads, hd), _heads(k, n, heads, hd), _heads(v, n, heads, hd), hd ** -0.5, causal=kind == "causal")
    flat = lambda t: t.transpose(1, 2).reshape(n * Nq, C)
    return q, k, v, flat(ref), flat(bound)


def _attn_launch(lib, kind, ld, ss):
    """one launch of attention kind `kind` with the row strides ld[name] / sample strides ss[name] given for q, k, v, o (others near);
    returns (rc, {name: FarGuarded}) -- the caller drops the buffers"""
    n, heads, hd, Nq, Nk = ATTN[kind]
    C = heads * hd
    q, k, v, _, _ = _attn_ref(kind)
    bufs = {}
    for name, t, N_ in (("q", q, Nq), ("k", k, Nk), ("v", v, Nk)):
        bufs[name] = U.guarded_far(t.reshape(n * N_, C).half(), ld.get(name, C + 64), samples=n, sstride=ss.get(name))
    bufs["o"] = out = U.guarded_far_out(n * Nq, C, ld.get("o", C + 8), samples=n, sstride=ss.get("o"))
    Q_, K_, V_ = bufs["q"], bufs["k"], bufs["v"]
    args = (Q_.ptr, K_.ptr, V_.ptr, out.ptr, Q_.ld, K_.ld, V_.ld, out.ld, Q_.sstride, K_.sstride, V_.sstride, out.sstride, n, heads)
    scale = hd ** -0.5
    if kind in ("flash", "flash_qb2"):
        rc = lib.ladi_op_attention(*args, Nq, Nk, scale, stream_ptr())
    elif kind == "causal":
        rc = lib.ladi_op_attention_causal(*args, Nq, Nk, scale, 1, stream_ptr())
    else:
        rc = lib.ladi_op_attention_generic(*args, hd, Nq, Nk, scale, stream_ptr())
    torch.cuda.synchronize()
    return rc, bufs


def _attn_judge(kind, bufs, what):
    _, _, _, ref, bound = _attn_ref(kind)
    ratio = U.check_elem(bufs["o"].cpu().float(), ref, bound, what)
    for name, g in bufs.items():
        U.assert_untouched_far(g, what + " " + name)
    return ratio


@pytest.mark.parametrize("far", ["ldq", "ldk", "ldv", "ldo", "sq", "sk", "sv", "so"])
@pytest.mark.parametrize("kind", ["flash", "flash_qb2", "causal", "generic"])
def test_attention_far_strides(lib, kind, far):
    """ladi_op_attention (both kernel forms: the 4 x 10 x 2600 x 300 shape takes the two-query-block one), _causal and _generic at the smallest
    shapes tests/test_gpu_views.py uses for them, one stride far at a time: a ROW stride that puts the operand's last row past 2^32 bytes, or
    a SAMPLE stride that puts the last sample 4 GiB behind the first.  (The K / V rows of one sample stay under the flash kernel's 2 GiB reach
    at these shapes -- the operand as a whole passes 2^32 --; test_flash_attention_kv_span_limit is about that reach.)"""
    n, heads, hd, Nq, Nk = ATTN[kind]
    name = far[-1]
    rows = n * (Nq if name in "qo" else Nk)
    ld = {name: FC.ld_for_bytes(rows, FC.MARK32)} if far.startswith("ld") else {}
    ss = {name: (FC.MARK32 // 2 + 64) // (n - 1) // 8 * 8 + 8} if far.startswith("s") else {}
    bufs = {}
    try:
        rc, bufs = _attn_launch(lib, kind, ld, ss)
        what = "attention_far %s %s" % (kind, far)
        assert rc == 0, (what, rc, _lib.last_error())
        reach = max(g.last_byte for g in bufs.values())
        assert reach > FC.MARK32, what
        _rec("attention_" + kind, far, _attn_judge(kind, bufs, what), reach)
    finally:
        bufs.clear()
        _release()


@pytest.mark.parametrize("far", ["k", "v"])
@pytest.mark.parametrize("kind", ["flash", "causal"])
def test_flash_attention_kv_span_limit(lib, kind, far):
    """the flash kernel streams the keys of one sample through 32-bit byte offsets from the sample's base: 2 ((Nk - 1) ld + 64) < 0x7FFFFFFF
    (include/ladi_native.h).  At the largest such row stride of K, then of V, the launch is right (two samples: the operand ends past 2^32
    bytes); one stride step above it is refused with rc -3 and a message, nothing launched, the output untouched.
    Measured before the refusal existed: rc 0 and 5548 (K) / 11594 (V) of 49152 elements outside the bound for the plain form, 86 / 113 of 19712
    for the causal one -- the last key's row read as zeros."""
    n, heads, hd, Nq, Nk = ATTN[kind]
    ld_max = ((FC.LIMIT - 1) // 2 - 64) // (Nk - 1) // 8 * 8
    assert 2 * ((Nk - 1) * ld_max + 64) < FC.LIMIT <= 2 * ((Nk - 1) * (ld_max + 8) + 64)
    for step, ld in (("below", ld_max), ("above", ld_max + 8)):
        bufs = {}
        try:
            rc, bufs = _attn_launch(lib, kind, {far: ld}, {})
            what = "flash_attention_kv_span %s %s %s" % (kind, far, step)
            if step == "below":
                assert rc == 0, (what, rc, _lib.last_error())
                _rec("attention_kv_span_" + kind, "%s-below" % far, _attn_judge(kind, bufs, what), max(g.last_byte for g in bufs.values()))
            else:
                assert rc == -3 and "span" in _lib.last_error(), (what, rc, _lib.last_error())
                FC.assert_nothing_written(bufs["o"], what)
                U.record_parity("far/attention_kv_span_%s[%s-above]" % (kind, far), dict(refused=rc, largest_byte_offset=int(bufs[far].last_byte)))
        finally:
            bufs.clear()
            _release()


@pytest.mark.parametrize("far", ["ldq", "ldvt", "ldo", "sq", "svt", "so"])
def test_attention_wide_far_strides(lib, far):
    """ladi_op_attention_wide at hd = 128, T = 17 (the small VAE-layout shape): q | k halves of one buffer (so ldq = ldk and sq = sk move together),
    V transposed [n][hd][ldvt], one stride far at a time"""
    n, hd, T = 2, 128, 17
    q, k, v = FC.rand((n, T, hd), 95), FC.rand((n, T, hd), 96), FC.rand((n, T, hd), 97)
    scale = hd ** -0.5
    ref, bound = U.attention_ref_bound(q, k, v, scale)
    far_s = FC.MARK32 // 2 + 64
    qk = vt = out = None
    try:
        qk = U.guarded_far(torch.cat([q, k], -1).reshape(n * T, 2 * hd).half(), FC.ld_for_bytes(n * T, FC.MARK32) if far == "ldq" else 2 * hd + 64,
                           samples=n, sstride=far_s if far == "sq" else None)
        vt = U.guarded_far(v.half().transpose(1, 2).reshape(n * hd, T), FC.ld_for_bytes(n * hd, FC.MARK32) if far == "ldvt" else 24,
                           samples=n, sstride=far_s if far == "svt" else None)
        out = U.guarded_far_out(n * T, hd, FC.ld_for_bytes(n * T, FC.MARK32) if far == "ldo" else hd + 8, samples=n, sstride=far_s if far == "so" else None)
        rc = lib.ladi_op_attention_wide(qk.col(0), qk.col(hd), vt.ptr, out.ptr, qk.ld, qk.ld, vt.ld, out.ld, qk.sstride, qk.sstride, vt.sstride, out.sstride,
                                        n, hd, T, T, scale, stream_ptr())
        torch.cuda.synchronize()
        what = "attention_wide_far " + far
        assert rc == 0, (what, rc, _lib.last_error())
        assert max(g.last_byte for g in (qk, vt, out)) > FC.MARK32
        ratio = U.check_elem(out.cpu().float(), ref.reshape(n * T, hd), bound.reshape(n * T, hd), what)
        for g, name in ((out, "output"), (qk, "qk"), (vt, "vt")):
            U.assert_untouched_far(g, what + " " + name)
        _rec("attention_wide", far, ratio, max(g.last_byte for g in (qk, vt, out)))
    finally:
        del qk, vt, out
        _release()


def test_scale_h16_and_pag_identity_far_rows(lib):
    """the two row-strided copy kernels: 200 rows of 320, source past 2^32 bytes and destination past 2^31, then swapped.  scale_h16 is
    fp16(float(x) * s), one fp32 product and one rounding: compared bit for bit, as tests/test_gpu_helpers.py does; pag_identity copies bits."""
    rows, C, s = 200, 320, 0.37
    x = FC.rand((rows, C), 610, 8.0).half()
    want = (x.float() * torch.tensor(s, dtype=torch.float32)).half()
    l31, l32 = _far_pair(rows)
    for case, lds, ldd in (("s32-d31", l32, l31), ("s31-d32", l31, l32)):
        X = out = None
        try:
            X = U.guarded_far(x, lds)
            for op in ("scale_h16", "pag_identity"):
                out = U.guarded_far_out(rows, C, ldd)
                if op == "scale_h16":
                    rc = lib.ladi_op_scale_h16(X.ptr, X.ld, out.ptr, out.ld, rows, C, s, stream_ptr())
                else:
                    rc = lib.ladi_op_pag_identity(X.ptr, X.ld, out.ptr, out.ld, rows, C, stream_ptr())
                torch.cuda.synchronize()
                what = "%s far %s" % (op, case)
                assert rc == 0, (what, rc, _lib.last_error())
                assert torch.equal(out.cpu().view(torch.int16), (want if op == "scale_h16" else x).view(torch.int16)), what
                U.assert_untouched_far(out, what + " output")
                U.assert_untouched_far(X, what + " input")
                _rec(op, case, 0.0, max(X.last_byte, out.last_byte))
                out = None
        finally:
            del X, out
            _release()


def test_image_post_far_rows(lib):
    """ladi_op_image_post: 384 pixels of 3 channels read at a row stride that puts the last pixel past 2^32 bytes; clip(x / 2 + 0.5, 0, 1) in fp32
    and round(255 v) as bytes, both exact against numpy (tests/helpers_cases.py image_post_ref, as tests/test_gpu_helpers.py compares)"""
    from tests import helpers_cases as HC
    n_pix = 384
    x = FC.rand((n_pix, 3), 620, 1.2).half()
    want_f, want_u = HC.image_post_ref(x)
    X = o32 = o8 = None
    try:
        X = U.guarded_far(x, FC.ld_for_bytes(n_pix, FC.MARK32))
        o32 = U.guarded_out(n_pix, 3, dtype=torch.float32, any_ld=True)
        o8 = torch.full((n_pix * 3 + 64,), 0xA5, dtype=torch.uint8, device=U.dev())
        assert lib.ladi_op_image_post(X.ptr, X.ld, n_pix, o32.ptr, 0, stream_ptr()) == 0, _lib.last_error()
        assert lib.ladi_op_image_post(X.ptr, X.ld, n_pix, ctypes.c_void_p(o8.data_ptr() + 32), 1, stream_ptr()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert X.last_byte > FC.MARK32
        assert torch.equal(o32.cpu(), want_f)
        U.assert_untouched(o32, "image_post_far fp32 output")
        U.assert_untouched_far(X, "image_post_far input")
        b = o8.cpu()
        assert bool((b[:32] == 0xA5).all()) and bool((b[32 + 3 * n_pix:] == 0xA5).all()) and torch.equal(b[32:32 + 3 * n_pix].reshape(n_pix, 3), want_u)
        _rec("image_post", "ld-far", 0.0, X.last_byte)
    finally:
        del X, o32, o8
        _release()


def _far_strides(far, name, rows, n):
    """(ld, sample stride) of operand `name` when `far` names its row stride ("ld" + name: the last row past 2^32 bytes) or its sample stride
    ("s" + name: the last of n samples 4 GiB behind the first); (None, None) = near"""
    if far == "ld" + name:
        return FC.ld_for_bytes(rows, FC.MARK32), None
    if far == "s" + name:
        return None, (FC.MARK32 // 2 + 64) // (n - 1) // 8 * 8 + 8
    return None, None


@pytest.mark.parametrize("far", ["ldq", "sq", "ldkv", "skv", "ldo", "so"])
def test_ip_attn_add_far_strides(lib, far):
    """ladi_op_ip_attn_add (o += scale softmax(q k^T / 8) v, in place) at n = 3, T = 5, 5 heads, N = 4 image tokens (tests/ip_adapter_cases.py),
    k | v the halves of one buffer: one row or sample stride far at a time"""
    import ctypes as ct
    from tests import ip_adapter_cases as IC
    c = (3, 5, 5, 4, 8, 0.6, "plain")
    n, T, heads, N, _, scale, _ = c
    Cc = heads * 64
    case = IC.make_case(*c)
    gq = gk = go = None
    try:
        ld, ss = _far_strides(far, "q", n * T, n)
        gq = U.guarded_far(case["q"].reshape(n * T, Cc), ld or Cc + 8, samples=n, sstride=ss)
        ld, ss = _far_strides(far, "kv", n * N, n)
        gk = U.guarded_far(case["kv"].reshape(n * N, 2 * Cc), ld or 2 * Cc + 8, samples=n, sstride=ss)
        ld, ss = _far_strides(far, "o", n * T, n)
        go = U.guarded_far(case["o"].reshape(n * T, Cc), ld or Cc + 8, samples=n, sstride=ss)
        rc = lib.ladi_op_ip_attn_add(ct.c_void_p(gq.ptr), gq.ld, gq.sstride, ct.c_void_p(gk.ptr), gk.ld, gk.sstride, ct.c_void_p(gk.col(Cc)), gk.ld, gk.sstride,
                                     ct.c_void_p(go.ptr), go.ld, go.sstride, n, heads, T, N, scale, stream_ptr())
        torch.cuda.synchronize()
        what = "ip_attn_add_far " + far
        assert rc == 0, (what, rc, _lib.last_error())
        reach = max(g.last_byte for g in (gq, gk, go))
        assert reach > FC.MARK32, what
        ratio = U.check_elem(go.cpu().reshape(n, T, Cc).float(), case["ref"], case["bound"], what)
        for g, name in ((gq, "q"), (gk, "k | v"), (go, "o")):
            U.assert_untouched_far(g, what + " " + name)
        assert torch.equal(gq.cpu(), case["q"].reshape(n * T, Cc)) and torch.equal(gk.cpu(), case["kv"].reshape(n * N, 2 * Cc)), what + ": inputs changed"
        _rec("ip_attn_add", far, ratio, reach)
    finally:
        del gq, gk, go
        _release()


@pytest.mark.parametrize("far", ["ld_h", "ld_s", "ld_d"])
def test_freeu_far_rows(lib, far):
    """ladi_op_freeu at n = 2, 3 x 2 pixels, C_h = 16, C_s = 8 (the smallest site of tests/test_gpu_freeu.py), out of place: the backbone rows,
    the skip rows or the filtered skip's rows at a stride that puts the last of the 12 rows past 2^32 bytes.  Judged as there: the scaled
    backbone half bit for bit, the untouched half and the source bit for bit, the filtered skip within test_gpu_freeu._check_skip's limit."""
    from tests import freeu_ref as R
    from tests import test_gpu_freeu as TF
    n, H, W, C_h, C_s, b, s_ = 2, 3, 2, 16, 8, 1.4, 0.9
    g = torch.Generator().manual_seed(4321)
    xh, xs = (torch.randn((n, H, W, C_h), generator=g) + 3.0).half(), (torch.randn((n, H, W, C_s), generator=g) + 3.0).half()
    lp = R.low_pass(xs.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    rows = n * H * W
    gh = gs = gd = None
    try:
        far_ld = FC.ld_for_bytes(rows, FC.MARK32)
        gh = U.guarded_far(xh, far_ld if far == "ld_h" else C_h + 8)
        gs = U.guarded_far(xs, far_ld if far == "ld_s" else C_s + 16)
        gd = U.guarded_far_out(rows, C_s, far_ld if far == "ld_d" else C_s + 8)
        rc = lib.ladi_op_freeu(gh.ptr, gh.ld, C_h, b, gs.ptr, gs.ld, C_s, s_, gd.ptr, gd.ld, n, H, W, stream_ptr())
        torch.cuda.synchronize()
        what = "freeu_far " + far
        assert rc == 0, (what, rc, _lib.last_error())
        got_h = gh.cpu().reshape(xh.shape)
        assert torch.equal(got_h[..., :C_h // 2], (xh[..., :C_h // 2].float() * b).half()), what
        assert torch.equal(got_h[..., C_h // 2:].contiguous().view(torch.int16), xh[..., C_h // 2:].contiguous().view(torch.int16)), what
        assert torch.equal(gs.cpu(), xs.reshape(-1, C_s)), what
        TF._check_skip(gd.cpu().reshape(xs.shape), xs, lp, s_, what)
        for gx, name in ((gh, "hidden"), (gs, "skip"), (gd, "skip_out")):
            U.assert_untouched_far(gx, what + " " + name)
        reach = max(gx.last_byte for gx in (gh, gs, gd))
        assert reach > FC.MARK32
        _rec("freeu", far, 0.0, reach)
    finally:
        del gh, gs, gd
        _release()


@pytest.mark.parametrize("far", ["ldx", "sx", "ldy", "sy"])
def test_tome_merge_far_strides(lib, far):
    """ladi_op_tome_merge at n = 2, 6 x 8 tokens, C = 64 (the smallest shape of tests/test_gpu_tome.py) with its supplied plan: the token rows x or
    the merged rows y at a far row or sample stride; against the float64 mean within that file's limit (2^-10 |ref| + 2^-24), unmerged rows
    copied bit for bit"""
    from tests import test_gpu_tome as TT
    n, h, w, Cc = TT.SHAPES[0]
    sp, dp, T, Ns, Nd = TT._geometry(h, w)
    r = int(0.6 * T) if int(0.6 * T) < Ns else Ns - 1
    Tm = T - r
    g = torch.Generator().manual_seed(T + Cc)
    x = (torch.randn((n, T, Cc), generator=g) * 2).half()
    plans = [TT._supplied_plan(sp, dp, 10 * s + T, r) for s in range(n)]
    dplan, ddp = TT._idev([v for p in plans for v in TT._plan_ints(p, Ns, Nd)]), TT._idev(dp)
    gx = gy = None
    try:
        ld, ss = _far_strides(far, "x", n * T, n)
        gx = U.guarded_far(x.reshape(n * T, Cc), ld or Cc + 8, samples=n, sstride=ss)
        ld, ss = _far_strides(far, "y", n * Tm, n)
        gy = U.guarded_far_out(n * Tm, Cc, ld or Cc + 16, samples=n, sstride=ss)
        rc = lib.ladi_op_tome_merge(gx.ptr, gx.ld, gx.sstride, ptr(ddp), ptr(dplan), n, T, Ns, Nd, r, Cc, gy.ptr, gy.ld, gy.sstride, stream_ptr())
        torch.cuda.synchronize()
        what = "tome_merge_far " + far
        assert rc == 0, (what, rc, _lib.last_error())
        out = gy.cpu().view(n, Tm, Cc)
        worst = 0.0
        for s in range(n):
            ref = TT.R.merge(x[s], plans[s], torch.float64)
            err, bound = (out[s].double() - ref).abs(), 2.0 ** -10 * ref.abs() + 2.0 ** -24
            assert bool(torch.isfinite(out[s]).all()) and bool((err <= bound).all()), (what, s, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            Nu = plans[s]["Nu"]
            assert torch.equal(out[s][:Nu].contiguous().view(torch.int16), x[s][plans[s]["unm"]].contiguous().view(torch.int16)), what
        assert torch.equal(gx.cpu(), x.reshape(n * T, Cc)), what
        U.assert_untouched_far(gx, what + " x")
        U.assert_untouched_far(gy, what + " y")
        reach = max(gx.last_byte, gy.last_byte)
        assert reach > FC.MARK32
        _rec("tome_merge", far, worst, reach)
    finally:
        del gx, gy
        _release()


@pytest.mark.parametrize("far", ["ldy", "sy", "ldr", "sr", "ldo", "so"])
def test_tome_unmerge_add_far_strides(lib, far):
    """ladi_op_tome_unmerge_add at the same shape: bit-equal to (y.float()[out_row] + res.float()).half() with the merged rows y, the residual
    or the output at a far row or sample stride"""
    from tests import test_gpu_tome as TT
    n, h, w, Cc = TT.SHAPES[0]
    sp, dp, T, Ns, Nd = TT._geometry(h, w)
    r = int(T / 2)
    Tm = T - r
    g = torch.Generator().manual_seed(T * Cc)
    y, res = (torch.randn((n, Tm, Cc), generator=g) * 3).half(), (torch.randn((n, T, Cc), generator=g) * 3).half()
    rows = torch.stack([TT._supplied_plan(sp, dp, s + T, r)["out_row"] for s in range(n)])
    drow = TT._idev(rows)
    want = torch.stack([(y[s].float()[rows[s]] + res[s].float()).half() for s in range(n)])
    gy = gr = go = None
    try:
        ld, ss = _far_strides(far, "y", n * Tm, n)
        gy = U.guarded_far(y.reshape(n * Tm, Cc), ld or Cc + 8, samples=n, sstride=ss)
        ld, ss = _far_strides(far, "r", n * T, n)
        gr = U.guarded_far(res.reshape(n * T, Cc), ld or Cc + 24, samples=n, sstride=ss)
        ld, ss = _far_strides(far, "o", n * T, n)
        go = U.guarded_far_out(n * T, Cc, ld or Cc + 16, samples=n, sstride=ss)
        rc = lib.ladi_op_tome_unmerge_add(gy.ptr, gy.ld, gy.sstride, gr.ptr, gr.ld, gr.sstride, ptr(drow), n, T, Tm, Cc, go.ptr, go.ld, go.sstride, stream_ptr())
        torch.cuda.synchronize()
        what = "tome_unmerge_add_far " + far
        assert rc == 0, (what, rc, _lib.last_error())
        assert torch.equal(go.cpu().view(n, T, Cc).view(torch.int16), want.view(torch.int16)), what
        assert torch.equal(gy.cpu(), y.reshape(-1, Cc)) and torch.equal(gr.cpu(), res.reshape(-1, Cc)), what
        for gx, name in ((gy, "y"), (gr, "res"), (go, "out")):
            U.assert_untouched_far(gx, what + " " + name)
        reach = max(gx.last_byte for gx in (gy, gr, go))
        assert reach > FC.MARK32
        _rec("tome_unmerge_add", far, 0.0, reach)
    finally:
        del gy, gr, go
        _release()


# ---------------------------------------------------------------------------------------------------------------------- dense, true size
def test_group_norm_true_size_past_4_gib(lib):
    """ladi_op_group_norm takes dense tensors only, and the product reaches 3.2 GB with it: C = 256 at 512 x 384 pixels, 43 samples = 4.33e9
    bytes in, as much out.  The one place where the reference runs on the device: torch in float64, sample by sample, with the bound formula
    of tests/util.py group_norm_ref_bound evaluated there too.  Input: N(0.5, 2) like the views test, a different seed per sample."""
    n, C, H, W, groups, eps = 43, 256, 512, 384, 32, 1e-5
    HW = H * W
    assert n * HW * C * 2 > FC.MARK32
    dev = U.dev()
    gam, bet = (FC.rand((C,), 33, 0.1) + 1).half(), FC.rand((C,), 34, 0.1).half()
    x = out = None
    try:
        x = torch.empty((n, HW, C), dtype=torch.float16, device=dev)
        gen = torch.Generator(device=dev)
        for s in range(n):
            gen.manual_seed(7000 + s)
            x[s] = (torch.randn((HW, C), generator=gen, device=dev, dtype=torch.float32) * 2.0 + 0.5 + 0.25 * s).half()
        out = torch.full((n, HW, C), float("nan"), dtype=torch.float16, device=dev)
        G, B = gam.to(dev), bet.to(dev)
        stats = torch.empty((n * groups * 2,), dtype=torch.float32, device=dev)
        rc = lib.ladi_op_group_norm(x.data_ptr(), C, None, 0, n, HW, groups, ptr(G), ptr(B), eps, 1, None, out.data_ptr(), ptr(stats), stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        g64, b64 = gam.double().to(dev).reshape(1, C), bet.double().to(dev).reshape(1, C)
        worst = 0.0
        for s in range(n):
            ratio = _gn_sample_ratio(x[s], out[s], g64, b64, groups, eps)
            assert ratio <= 1.0, "group_norm true size: sample %d (byte offset %d) is off by %.3f of its limit" % (s, s * HW * C * 2, ratio)
            worst = max(worst, ratio)
        _rec("group_norm", "43x512x384x256", worst, n * HW * C * 2 - 1)
    finally:
        del x, out
        _release()


def _gn_sample_ratio(xs, got, g64, b64, groups, eps):
    """worst |got - ref| / (ulp16(ref) + bound) of one sample [HW, C] on the device: tests/util.py group_norm_ref_bound (with SiLU) in torch
    float64, group by group of the channels so that the float64 temporaries stay at HW x C / groups"""
    HW, C = xs.shape
    cg = C // groups
    worst = torch.zeros((), dtype=torch.float64, device=xs.device)
    nel = HW * cg
    for g0 in range(groups):
        sl = slice(g0 * cg, (g0 + 1) * cg)
        x = xs[:, sl].double()
        m = x.mean()
        v = ((x - m) ** 2).mean()
        e_m = (nel + 1) * U.U32 * x.abs().mean()
        e_v = (nel + 3) * U.U32 * (x * x).mean() + 2 * m.abs() * e_m
        r = torch.rsqrt(v + eps)
        dr = r * e_v / (2 * (v + eps)) + 2 * U.U32 * r
        gm, bt = g64[:, sl], b64[:, sl]
        scale, shift = r * gm, bt - m * r * gm
        y = x * scale + shift
        dscale = gm.abs() * dr + U.U32 * scale.abs()
        dshift = gm.abs() * (e_m * r + m.abs() * dr) + 3 * U.U32 * ((m * r * gm).abs() + bt.abs())
        e = x.abs() * dscale + dshift + 2 * U.U32 * ((x * scale).abs() + shift.abs())
        t = F.silu(y)
        e = U.ACT_LIP["silu"] * e + U.ACT_EVAL * t.abs()
        lim = U.ulp16(t) + e
        o = got[:, sl].double()
        assert bool(torch.isfinite(o).all()), "non-finite output in channel group %d" % g0
        worst = torch.maximum(worst, ((o - t).abs() / lim).max())
    return float(worst)


def test_nhwc_to_nchw_true_size_past_4_gib(lib):
    """ladi_op_nhwc_to_nchw, C = 256 at 512 x 384, 43 samples: 4.33e9 bytes of fp16 in, the same out (dtype 1 = fp16).  A layout change: exact, compared
    on the device sample by sample.  The input holds a pattern that names its own position (sample, pixel and channel folded into an integer below 2039, exact in fp16), so a wrapped offset cannot land on an equal value."""
    n, C, H, W = 43, 256, 512, 384
    HW = H * W
    dev = U.dev()
    x = out = None
    try:
        p = torch.arange(HW, device=dev, dtype=torch.int32).reshape(HW, 1)
        c = torch.arange(C, device=dev, dtype=torch.int32).reshape(1, C)
        x = torch.empty((n, HW, C), dtype=torch.float16, device=dev)
        for s in range(n):
            x[s] = ((p * 7 + c * 13 + s * 101) % 2039).half()
        out = torch.full((n, C, HW), float("nan"), dtype=torch.float16, device=dev)
        rc = lib.ladi_op_nhwc_to_nchw(x.data_ptr(), C, n, C, H, W, out.data_ptr(), 1, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        for s in range(n):
            assert torch.equal(out[s], x[s].t()), "nhwc_to_nchw true size: sample %d (byte offset %d) differs" % (s, s * HW * C * 2)
        _rec("nhwc_to_nchw", "43x512x384x256", 0.0, n * HW * C * 2 - 1)
    finally:
        del x, out
        _release()
