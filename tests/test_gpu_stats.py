"""Fused GroupNorm statistics, writer by writer and reader by reader.

Nearly every GroupNorm of the UNet and the VAE takes its statistics from the epilogue of the convolution that produced its input: conv2d()
(runtime_core.cpp) passes a.stats, the igemm epilogue writes per-channel partial rows [row][Q][2] (sum, sum of squares of the values as
stored), ladi_launch_igemm reports the pixels per row, and group_norm() hands HW / px rows per sample to gn_norm, gn_reduce + gn_norm or
gn_finalize + gn_apply.  Four writers (igemm_epilogue_fast, igemm_epilogue_generic, the in-launch split-K combine, splitk_reduce_kernel), three
readers, and the launcher's silent demotions in between (the X-stationary kernel, HW % px != 0, GEGLU, batched launches, fp32 output).

Here every launch names its configuration and writes into a NaN-poisoned statistics buffer between guard rows:
  * the output is judged element by element against the float64 reference (tests/test_gpu_views.py ConvProblem.check), and the rows against
    the statistics of the output the launch actually stored (tests/stats_cases.py judge_rows, tests/util.py stats_rows_ref_bound): exactly
    n HW / px rows, every channel of them finite, rows [s rps, (s + 1) rps) adding up to sample s, everything else still poison, and a
    repeat launch gives the same bits;
  * a demoted launch reports 0 and leaves the buffer bit-identical;
  * the readers run, through the runtime's own group_norm() (ladi_op_group_norm_rows), on synthetic rows of the heights producers give and
    on the rows a producer has just written (the chain).
The worst err / limit of every case goes to the parity record under "stats/..." keys."""
import ctypes
import functools

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from tests import stats_cases as S
from tests import util as U
from tests.test_gpu_views import SYMBOL_FAMILY, _cfg_tile, _geglu_pack, _kw, _last_launch, _problem_kw

pytestmark = pytest.mark.gpu


def _record(test, case, ratio):
    assert ratio <= 1.0, (test, case, ratio)
    U.record_parity("stats/%s[%s]" % (test, case), round(ratio, 4))


def _problem(spec):
    args, kw = spec
    return _problem_kw(args, _kw(**kw))


def _symbol(lib, cfg):
    return lib.ladi_igemm_cfg_symbol_name(cfg).decode()


def _is_xs(lib, cfg):
    return SYMBOL_FAMILY[_symbol(lib, cfg).split("<")[0]] == "linear_xs"


def _desc(pb, out_ptr, ldo, stats=None, res=None):
    """ConvProblem.try_launch's descriptor, with a statistics buffer and (res = Guarded) another placement of the residual"""
    d = _lib.IGemmDesc()
    d.src0, d.C0, d.ld0 = pb.X0.ptr, pb.C0p, pb.X0.ld
    if pb.X1 is not None:
        d.src1, d.C1, d.ld1 = pb.X1.ptr, pb.C1p, pb.X1.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = pb.h, pb.w, pb.Ho, pb.Wo, pb.P
    d.ksize, d.stride, d.pad, d.ups = pb.ksize, pb.stride, pb.pad, pb.ups
    d.W, d.Q, d.K, d.ldw = pb.W.data_ptr(), pb.cout, pb.ksize * pb.ksize * (pb.C0p + (pb.C1p if pb.X1 is not None else 0)), 0
    d.bias, d.act, d.out_scale = pb.B.data_ptr(), U.ACT[pb.act], 1.0
    if pb.TE is not None:
        d.rowadd = pb.TE.data_ptr()
    r = res if res is not None else pb.R
    if r is not None:
        d.res0, d.ldr0 = r.ptr, r.ld
    if pb.M is not None:
        d.mask = pb.M.ptr
    d.out, d.ldo = out_ptr, ldo
    if stats is not None:
        d.stats = stats.ptr
    return d


def _run(lib, pb, cfg, res=None, out_ld=None):
    """one ladi_op_igemm_stats launch into a fresh poisoned output and a fresh poisoned statistics buffer; (rc, reported px, output, rows)"""
    ldo = out_ld or pb.cout + 8
    out = U.guarded_out(pb.P, pb.cout, ld=ldo, pre_rows=4, post_rows=4)
    st = S.poisoned_rows(pb.P, pb.cout)
    d = _desc(pb, out.ptr, ldo, st, res)
    px = ctypes.c_int(-1)
    rc = lib.ladi_op_igemm_stats(ctypes.byref(d), 1, cfg, ctypes.byref(px), stream_ptr())
    torch.cuda.synchronize()
    return rc, px.value, out, st


def _judge(lib, pb, cfg, what, res=None, out_ld=None):
    """a launch of cfg on pb, judged as the file's docstring says; None when the launcher refuses it, else dict(px, info, ratio, out, st)"""
    rc, px, out, st = _run(lib, pb, cfg, res, out_ld)
    if rc != 0:
        assert rc < 0 and px == 0, (what, rc, px)
        S.assert_all_poison(st, what + " (refused, rc = %d)" % rc)
        return None
    info = _last_launch(lib)
    what = "%s %s" % (what, info)
    pb.check(lib, cfg, out, what)
    if res is not None:
        U.assert_untouched(res, what + " input res")
    HW = pb.Ho * pb.Wo
    ratio = 0.0
    if px == 0:
        S.assert_all_poison(st, what + " (reported px = 0)")
    else:
        ratio = S.judge_rows(st, px, out.cpu().double(), pb.N, HW, what + " px %d" % px)
        rc2, px2, out2, st2 = _run(lib, pb, cfg, res, out_ld)
        assert rc2 == 0 and px2 == px, (what, rc2, px2)
        assert torch.equal(st2._bits(), st._bits()), what + ": the rows of a repeat launch differ"
        assert torch.equal(out2._bits(), out._bits()), what + ": the output of a repeat launch differs"
    return dict(px=px, info=info, ratio=ratio, out=out, st=st)


class _two_pass:
    """the split-K form of the launches inside: the separate reduce pass (on) or the in-launch combine, the default, restored on the way out"""

    def __init__(self, lib, on):
        self.lib, self.on = lib, on

    def __enter__(self):
        self.lib.ladi_igemm_set_splitk_two_pass(1 if self.on else 0)

    def __exit__(self, *exc):
        self.lib.ladi_igemm_set_splitk_two_pass(0)


# ---------------------------------------------------------------------------------------------------------------------- producers
_SWEEPS = {}
# the split factors test_gpu_views.py test_conv3x3_split_k pins, for the configurations the split-K problem reaches
KNOWN_SPLIT = {14: 2, 12: 4, 36: 2, 69: 2, 80: 2, 86: 2, 90: 2, 109: 8}


def _sweep(lib, name, two_pass=False):
    """every configuration on one problem of tests/stats_cases.py SWEEP (once per session): {cfg: dict(px, split)} of the accepted launches.
    A tiled configuration must report the row height of its kernel form (stats_cases.expected_row_px: 32 TP, 32 for the two-pass split-K
    reduce) -- which is 0, with an untouched buffer, only where a sample is not a whole number of such rows: the 256-pixel samples of the
    2-D blocked problem on the 96-pixel rows of the TP = 3 forms (the launcher's HW % px demotion).  The X-stationary kernel reports 0."""
    key = (name, two_pass)
    if key in _SWEEPS:
        return _SWEEPS[key]
    pb = _problem(S.sweep_problem(name))
    HW = pb.Ho * pb.Wo
    got, worst = {}, 0.0
    with _two_pass(lib, two_pass):
        for cfg in range(1, lib.ladi_igemm_cfg_count() + 1):
            r = _judge(lib, pb, cfg, "sweep %s%s cfg %d" % (name, " two-pass" if two_pass else "", cfg))
            if r is None:
                continue
            split = r["info"]["split"]
            expect = S.expected_row_px(_symbol(lib, cfg), split, two_pass, HW)
            assert r["px"] == expect, "sweep %s cfg %d %s: reported rows of %d pixels, its form %s writes rows of %d" % (
                name, cfg, r["info"], r["px"], _symbol(lib, cfg), expect)
            assert _is_xs(lib, cfg) == (r["info"]["family"] == "linear_xs")
            if not _is_xs(lib, cfg) and HW % 96 == 0:
                assert r["px"] > 0 and HW % r["px"] == 0, (name, cfg, r["px"])
            if split > 1 and two_pass:
                assert r["px"] == 32, (name, cfg, r["px"])
            got[cfg] = dict(px=r["px"], split=split)
            worst = max(worst, r["ratio"])
    assert any(v["px"] > 0 for v in got.values()), "no configuration wrote statistics on problem %s" % name
    _record("sweep", name + ("-twopass" if two_pass else ""), worst)
    _SWEEPS[key] = got
    return got


@pytest.mark.parametrize("name", [n for n in S.SWEEP_NAMES if n != "splitk"])
def test_every_configuration_writes_the_rows_it_reports(lib, name):
    """the producer sweep: every tile configuration 1..ladi_igemm_cfg_count() on the problem, refusals skipped (see _sweep and _judge)"""
    got = _sweep(lib, name)
    families = {SYMBOL_FAMILY[_symbol(lib, c).split("<")[0]] for c, v in got.items() if v["px"] > 0}
    need = dict(ragged={"ring", "igemm8", "igemm_lc", "halo"}, halo2d={"ring", "igemm8", "igemm_lc", "halo"}, stride2={"ring", "igemm8", "igemm_lc"},
                upsample={"ring", "igemm8", "halo"})
    need["1x1res"] = {"ring", "igemm8", "igemm_lc"}
    assert need[name] <= families, (name, families)
    if name == "halo2d":
        assert all(c in got and got[c]["px"] > 0 for c in (100, 101, 102, 103)), {c: got.get(c) for c in (100, 101, 102, 103)}
    if name == "upsample":
        assert any(c in got and got[c]["px"] > 0 for c in (104, 105, 106, 107, 108)), got


@pytest.mark.parametrize("two_pass", [False, True])
def test_split_k_rows_in_both_forms(lib, two_pass):
    """N = 2, 512 -> 192 at 16 x 24 (SiLU + time embedding + residual) on every configuration, once per split-K form: the in-launch combine's
    last-arriving slice writes rows of 32 TP pixels like the plain epilogue, the two-pass reduce rows of 32 pixels.  The split the launch
    reports is the configuration's (the factors test_gpu_views.py pins) and does not depend on the form."""
    got = _sweep(lib, "splitk", two_pass)
    for cfg, split in KNOWN_SPLIT.items():
        assert cfg in got and got[cfg]["split"] == split, (cfg, got.get(cfg))
    splits = {c: v for c, v in got.items() if v["split"] > 1}
    assert len(splits) >= len(KNOWN_SPLIT) and all(v["px"] > 0 for v in splits.values()), splits
    if two_pass:
        assert all(v["px"] == 32 for v in splits.values()), splits
    else:
        assert any(v["px"] > 32 for v in splits.values()), "no in-launch split-K row of more than 32 pixels: %s" % splits
    other = _sweep(lib, "splitk", not two_pass)
    assert {c: v["split"] for c, v in got.items()} == {c: v["split"] for c, v in other.items()}


def test_every_tiled_configuration_writes_statistics_on_some_problem(lib):
    """coverage of the sweep: no configuration but the X-stationary ones may go without a problem on which it writes statistics"""
    wrote = set()
    for name in S.SWEEP_NAMES:
        wrote |= {c for c, v in _sweep(lib, name).items() if v["px"] > 0}
    n = lib.ladi_igemm_cfg_count()
    missing = [c for c in range(1, n + 1) if not _is_xs(lib, c) and c not in wrote]
    assert not missing, "tiled configurations that wrote statistics on no problem of the sweep: %s" % missing
    for name in S.SWEEP_NAMES:
        for c, v in _sweep(lib, name).items():
            assert not (_is_xs(lib, c) and v["px"]), (name, c, v)
    assert any(_is_xs(lib, c) for c in _sweep(lib, "1x1res")), "the X-stationary kernel accepted no problem: its demotion went unseen"


@pytest.mark.parametrize("cfg", [3, 32, 74])
def test_generic_epilogue_rows(lib, cfg):
    """a residual at ldr0 = Q + 4 (no multiple of 8) takes the workgroup to igemm_epilogue_generic: scalar residual reads, per-element statistics
    stores; one ring, one igemm8 and one halo configuration on the ragged problem (Q = 96)"""
    pb = _problem(S.sweep_problem("ragged"))
    res = _generic_residual()
    assert res.ld == pb.cout + 4 and res.ld % 8 == 4
    r = _judge(lib, pb, cfg, "generic epilogue cfg %d" % cfg, res=res)
    assert r is not None and r["px"] == S.expected_row_px(_symbol(lib, cfg), 1, False, pb.Ho * pb.Wo) > 0, r
    _record("generic_epilogue", "cfg%d" % cfg, r["ratio"])


@functools.lru_cache(maxsize=None)
def _generic_residual():
    pb = _problem(S.sweep_problem("ragged"))
    guard = pb.Wo + 2
    return U.guarded(pb.R.view[:, :pb.cout].contiguous(), ld=pb.cout + 4, pre_rows=guard, post_rows=guard)


# ---------------------------------------------------------------------------------------------------------------------- demotions
DEMOTION_CFGS = [3, 32, 62, 74]


def _demoted(what, rc, px, st):
    """rc 0 or a refusal; either way no rows are reported and the statistics buffer is bit-identical"""
    assert rc <= 0 and px == 0, "%s: rc = %d, reported rows of %d pixels" % (what, rc, px)
    S.assert_all_poison(st, what)
    return rc == 0


def _demotion_samples_that_are_no_whole_rows(lib, cfg):
    """8 x 6 samples: 48 pixels are no multiple of any row height"""
    pb = _problem(S.SMALL_SAMPLES)
    rc, px, out, st = _run(lib, pb, cfg)
    what = "demotion 8x6 cfg %d" % cfg
    if _demoted(what, rc, px, st):
        return pb.check(lib, cfg, out, what)


def _demotion_batched_launch(lib, cfg):
    """batch = 3 (shared operands, three outputs one behind the other): no statistics, three correct outputs"""
    pb = _problem(S.PLAIN)
    ldo = pb.cout + 8
    out = U.guarded_out(3 * pb.P, pb.cout, ld=ldo, pre_rows=4, post_rows=4)
    st = S.poisoned_rows(3 * pb.P, pb.cout)
    d = _desc(pb, out.ptr, ldo, st)
    d.bs_out = pb.P * ldo
    px = ctypes.c_int(-1)
    rc = lib.ladi_op_igemm_stats(ctypes.byref(d), 3, cfg, ctypes.byref(px), stream_ptr())
    torch.cuda.synchronize()
    what = "demotion batch 3 cfg %d" % cfg
    if _demoted(what, rc, px.value, st):
        got = out.cpu().float().reshape(3, pb.P, pb.cout)
        ratio = max(U.check_elem(got[b], pb.ref, pb.bound, "%s element %d" % (what, b), U.pixel_locator(pb.N, pb.Ho, pb.Wo, pb.cout)) for b in range(3))
        U.assert_untouched(out, what + " output")
        return ratio


def _demotion_fp32_output(lib, cfg):
    """out_f32: the store is (acc + bias) in fp32, no statistics"""
    pb = _problem(S.PLAIN)
    ldo = pb.cout + 8
    out = U.guarded_out(pb.P, pb.cout, ld=ldo, pre_rows=4, post_rows=4, dtype=torch.float32)
    st = S.poisoned_rows(pb.P, pb.cout)
    d = _desc(pb, out.ptr, ldo, st)
    d.out_f32 = 1
    px = ctypes.c_int(-1)
    rc = lib.ladi_op_igemm_stats(ctypes.byref(d), 1, cfg, ctypes.byref(px), stream_ptr())
    torch.cuda.synchronize()
    what = "demotion out_f32 cfg %d" % cfg
    if _demoted(what, rc, px.value, st):
        ratio = U.check_elem(out.cpu(), pb.ref, pb.bound, what, U.pixel_locator(pb.N, pb.Ho, pb.Wo, pb.cout), out_f32=True)
        U.assert_untouched(out, what + " output")
        return ratio


@functools.lru_cache(maxsize=None)
def _geglu_problem():
    """a GEGLU projection, 128 -> 2 x 64 on N = 2 samples of 16 x 24 pixels (1x1): value and gate rows in the kernels' 32-row packing"""
    n, h, w, C, Q = 2, 16, 24, 128, 128
    x, wt, b = S.rand((n * h * w, C), 900), S.rand((Q, C), 901, C ** -0.5), S.rand((Q,), 902, 0.1)
    ref, bound = U.geglu_ref_bound(x, wt, b)
    wp, bp = _geglu_pack(wt, b)
    return dict(n=n, h=h, w=w, C=C, Q=Q, P=n * h * w, ref=ref, bound=bound, X=U.guarded(x.half(), ld=C + 64, pre_rows=w + 2, post_rows=w + 2),
                W=wp.half().contiguous().to(U.dev()), B=bp.half().to(U.dev()))


def _demotion_geglu(lib, cfg):
    """GEGLU halves the channels in the epilogue: no statistics"""
    g = _geglu_problem()
    Qo = g["Q"] // 2
    out = U.guarded_out(g["P"], Qo, ld=Qo + 8, pre_rows=4, post_rows=4)
    st = S.poisoned_rows(g["P"], g["Q"])
    d = _lib.IGemmDesc()
    d.src0, d.C0, d.ld0 = g["X"].ptr, g["C"], g["X"].ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = g["h"], g["w"], g["h"], g["w"], g["P"]
    d.ksize, d.stride, d.pad, d.ups = 1, 1, 0, 0
    d.W, d.Q, d.K, d.ldw = g["W"].data_ptr(), g["Q"], g["C"], 0
    d.bias, d.act, d.out_scale = g["B"].data_ptr(), U.ACT["geglu"], 1.0
    d.out, d.ldo, d.stats = out.ptr, Qo + 8, st.ptr
    px = ctypes.c_int(-1)
    rc = lib.ladi_op_igemm_stats(ctypes.byref(d), 1, cfg, ctypes.byref(px), stream_ptr())
    torch.cuda.synchronize()
    what = "demotion GEGLU cfg %d" % cfg
    if _demoted(what, rc, px.value, st):
        ratio = U.check_elem(out.cpu().float(), g["ref"], g["bound"], what, U.pixel_locator(g["n"], g["h"], g["w"], Qo))
        U.assert_untouched(out, what + " output")
        U.assert_untouched(g["X"], what + " input x")
        return ratio


DEMOTIONS = {"8x6": _demotion_samples_that_are_no_whole_rows, "batch3": _demotion_batched_launch, "out_f32": _demotion_fp32_output, "geglu": _demotion_geglu}


@pytest.mark.parametrize("case", sorted(DEMOTIONS))
def test_demoted_launches_report_no_rows_and_write_none(lib, case):
    """the launcher's silent demotions on one ring, igemm8, loader / consumer and halo configuration each: rc 0 or a refusal, px = 0, the
    statistics buffer bit-identical, and where the launch was accepted the output within its bound.  Every case is accepted by at least one
    configuration, so that the demotion is seen on a real launch."""
    accepted = 0
    for cfg in DEMOTION_CFGS:
        ratio = DEMOTIONS[case](lib, cfg)
        if ratio is not None:
            accepted += 1
            _record("demotion", "%s-cfg%d" % (case, cfg), ratio)
    assert accepted, "every configuration refused the %s case" % case


# ---------------------------------------------------------------------------------------------------------------------- consumers
FORMS = dict(default=None, no_reduce=("LADI_GN_REDUCE", "0"), no_onepass=("LADI_GN_ONEPASS", "0"))
ROW_GUARD = 4


@functools.lru_cache(maxsize=None)
def _consumer_dev(c0, c1, HW):
    c = S.consumer_case(c0, c1, HW)
    dense = lambda t: U.guarded(t.half(), pre_rows=8, post_rows=8)
    return dict(case=c, X0=dense(c.source(0)), X1=dense(c.source(1)) if c1 else None, AD=dense(c.add), G=c.gamma.half().to(U.dev()),
                B=c.beta.half().to(U.dev()))


@functools.lru_cache(maxsize=None)
def _consumer_rows(c0, c1, HW, i, px):
    return S.rows_buffer(S.consumer_case(c0, c1, HW).rows(i, px), ROW_GUARD) if px else None


def _group_norm_rows(lib, c0, c1, HW, px0, px1, silu, with_add, what):
    """one ladi_op_group_norm_rows call on the case's operands; returns (rc, output)"""
    dv = _consumer_dev(c0, c1, HW)
    c = dv["case"]
    r0, r1 = _consumer_rows(c0, c1, HW, 0, px0), (_consumer_rows(c0, c1, HW, 1, px1) if c1 else None)
    out = U.guarded_out(c.n * HW, c0 + c1, pre_rows=8, post_rows=8)
    rc = lib.ladi_op_group_norm_rows(dv["X0"].ptr, c0, r0.ptr if r0 else None, px0, dv["X1"].ptr if c1 else None, c1, r1.ptr if r1 else None, px1,
                                     c.n, HW, S.GROUPS, ptr(dv["G"]), ptr(dv["B"]), S.EPS, silu, dv["AD"].ptr if with_add else None, out.ptr, stream_ptr())
    torch.cuda.synchronize()
    return rc, out, [g for g in (dv["X0"], dv["X1"], dv["AD"], r0, r1) if g is not None]


def _consumer_judge(lib, test, case_name, c0, c1, HW, px0, px1, silu, with_add):
    c = S.consumer_case(c0, c1, HW)
    what = "%s %s silu %d add %d" % (test, case_name, silu, with_add)
    rc, out, inputs = _group_norm_rows(lib, c0, c1, HW, px0, px1, silu, with_add, what)
    assert rc == 0, "%s: rc = %d (%s)" % (what, rc, _lib.last_error())
    ref, bound = c.refs[(silu, with_add)]
    ratio = U.check_elem(out.cpu().float(), ref, bound, what, U.pixel_locator(c.n, HW, 1, c0 + c1))
    U.assert_untouched(out, what + " output")
    for g in inputs:
        U.assert_untouched(g, what + " input")
    rc, again, _ = _group_norm_rows(lib, c0, c1, HW, px0, px1, silu, with_add, what)
    assert rc == 0 and torch.equal(again.cpu(), out.cpu()), what + ": repeat differs"
    _record(test, "%s-silu%d-add%d" % (case_name, silu, int(with_add)), ratio)


@pytest.mark.parametrize("silu,with_add", [(0, False), (1, True)])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("HW,px", S.ONE_SOURCE)
def test_group_norm_on_producer_shaped_rows(lib, monkeypatch, HW, px, form, silu, with_add):
    """one source of 64 channels with rows of px pixels: rps = 1, 3, 4, 12 (what producers give at 384 pixels per sample), 96 (the one-pass
    kernel's limit), 97 (the first above it, no multiple of the fold's 16 rows), 510; through the default dispatch, without the fold
    (LADI_GN_REDUCE=0: gn_finalize + gn_apply above 96 rows) and without the one-pass kernel (LADI_GN_ONEPASS=0: always gn_finalize + gn_apply).
    The rows are float64 block sums rounded to fp32 between poison rows: a reader that walks past its rows returns NaN."""
    if FORMS[form]:
        monkeypatch.setenv(*FORMS[form])
    _consumer_judge(lib, "consumer_one_source", "hw%d-rps%d-%s" % (HW, HW // px, form), 64, 0, HW, px, 0, silu, with_add)


@pytest.mark.parametrize("silu,with_add", [(0, False), (1, True)])
@pytest.mark.parametrize("HW,px0,px1", S.TWO_SOURCES)
def test_group_norm_two_sources_with_different_rows(lib, HW, px0, px1, silu, with_add):
    """the two sources of an up block's GroupNorm, 320 + 160 channels (groups of 15 straddle the boundary): rows of different heights, rows on
    one side only (the other side's statistics from gn_partial), and at 64 pixels per sample the direct path (no rows, statistics from the data)"""
    _consumer_judge(lib, "consumer_two_sources", "hw%d-px%d+%d" % (HW, px0, px1), 320, 160, HW, px0, px1, silu, with_add)


def test_group_norm_rows_refuses_rows_it_cannot_use(lib):
    """rows that do not divide the sample, and a row height without a buffer: refused, nothing launched, the output untouched"""
    dv = _consumer_dev(64, 0, 384)
    c = dv["case"]
    rows = _consumer_rows(64, 0, 384, 0, 128)
    for part, px in ((rows.ptr, 256), (None, 128), (rows.ptr, -32)):
        out = U.guarded_out(c.n * 384, 64, pre_rows=8, post_rows=8)
        before = out._bits().clone()
        rc = lib.ladi_op_group_norm_rows(dv["X0"].ptr, 64, part, px, None, 0, None, 0, c.n, 384, S.GROUPS, ptr(dv["G"]), ptr(dv["B"]), S.EPS, 0, None,
                                         out.ptr, stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and torch.equal(out._bits(), before), (px, rc)
    dv2 = _consumer_dev(320, 160, 384)
    rows1 = _consumer_rows(320, 160, 384, 1, 32)
    out = U.guarded_out(dv2["case"].n * 384, 480, pre_rows=8, post_rows=8)
    before = out._bits().clone()
    for part, px in ((rows1.ptr, 256), (None, 32)):                  # the same on the second source
        rc = lib.ladi_op_group_norm_rows(dv2["X0"].ptr, 320, None, 0, dv2["X1"].ptr, 160, part, px, 2, 384, S.GROUPS, ptr(dv2["G"]), ptr(dv2["B"]), S.EPS, 0,
                                         None, out.ptr, stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and torch.equal(out._bits(), before), (px, rc)


# ---------------------------------------------------------------------------------------------------------------------- chain
CHAIN = [(3, "ragged", False), (32, "ragged", False), (62, "ragged", False), (84, "ragged", False), (101, "halo2d", False), (14, "splitk", False),
         (14, "splitk", True)]


@pytest.mark.parametrize("cfg,name,two_pass", CHAIN)
def test_conv_rows_feed_group_norm(lib, cfg, name, two_pass):
    """producer -> reader: a convolution with statistics into a dense output, then ladi_op_group_norm_rows with the row height the launch
    reported, SiLU; judged against the float64 GroupNorm of the conv output as stored.  One configuration per family on its problem of the
    sweep, split-K in both forms."""
    pb = _problem(S.sweep_problem(name))
    HW, Q = pb.Ho * pb.Wo, pb.cout
    what = "chain cfg %d %s%s" % (cfg, name, " two-pass" if two_pass else "")
    with _two_pass(lib, two_pass):
        r = _judge(lib, pb, cfg, what, out_ld=Q)
    assert r is not None and r["px"] > 0, (what, r)
    stored = r["out"].cpu().float()                                                  # [P, Q]
    gam, bet = (S.rand((Q,), 950, 0.1) + 1).half().float(), S.rand((Q,), 951, 0.1)
    x4 = stored.reshape(pb.N, HW, 1, Q).permute(0, 3, 1, 2)
    ref, bound = U.group_norm_ref_bound(x4, S.GROUPS, gam, bet, S.EPS, silu=True)
    G, B = gam.half().to(U.dev()), bet.half().to(U.dev())
    out = U.guarded_out(pb.P, Q, pre_rows=8, post_rows=8)
    rc = lib.ladi_op_group_norm_rows(r["out"].ptr, Q, r["st"].ptr, r["px"], None, 0, None, 0, pb.N, HW, S.GROUPS, ptr(G), ptr(B), S.EPS, 1, None, out.ptr,
                                     stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, "%s: rc = %d (%s)" % (what, rc, _lib.last_error())
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(pb.P, Q)
    ratio = U.check_elem(out.cpu().float(), flat(ref), flat(bound), what, U.pixel_locator(pb.N, pb.Ho, pb.Wo, Q, *_cfg_tile(lib, cfg)))
    U.assert_untouched(out, what + " output")
    U.assert_untouched(r["out"], what + " conv output")
    U.assert_untouched(r["st"], what + " rows")
    _record("chain", "cfg%d-%s%s" % (cfg, name, "-twopass" if two_pass else ""), max(ratio, r["ratio"]))
