"""Activations over every finite fp16 input and norms where eps, the variance clamp and zero decide (data, references and bounds:
tests/numeric_edge_cases.py; the judges are shown to be able to fail in tests/test_cpu_numeric_edges.py).

A. Each place of the library that evaluates an activation is swept over all 63 488 finite halves and three points between neighbours, the
pre-activation produced exactly by selection-matrix weights, and judged with check_elem against the float64 activation and tests/util.py's
ACT_EVAL / GELU_ERF_ABS allowance alone.  Which code a launch ran is read off what the library reports: the family and split of the last launch
(ladi_igemm_last_launch), the kernel symbol of the configuration (ladi_igemm_cfg_symbol_name), the statistics-row height that tells the two
split-K forms apart (32 pixels: splitk_reduce_kernel, 32 TP: the in-launch combine), and the epilogue's own workgroup-uniform dispatch
condition (igemm_common.h igemm_epilogue: fp16 rows with ld % 8 == 0 and Q % 8 == 0 take igemm_epilogue_fast, everything else the generic one).

B. Every norm entry point on inputs of variance ~1.5e-5 (eps decides 25-60 % of rstd), on constant groups / rows (variance 0: the one-pass
form's clamp) and on zeros, each with eps = 1e-5 and 1e-6.  The op-level entry points pass no `bad` flag to the kernels (it belongs to the
VAE's context), so what is asserted for the constant and zero families is a finite output inside the bound.

Every case records its worst err / limit (and, for the sweeps, the x where it occurs) under numeric_edges/... in the parity file."""
import ctypes
import functools

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ConvF32Desc, ptr, stream_ptr
from tests import helpers_cases as HC
from tests import numeric_edge_cases as NE
from tests import stats_cases as S
from tests import util as U

pytestmark = pytest.mark.gpu

FAMILY = {1: "ring", 2: "igemm8", 3: "igemm_lc", 4: "halo", 5: "linear_xs"}
RING = 3            # igemm_kernel<2, 2, 2, 2, ...>: TQ = 2, GEGLU-capable
RING_ODD_TQ = 5     # igemm_kernel<2, 2, 1, 1, ...>: TQ = 1
SPLITK = 14         # cfg 7 (igemm_kernel<2, 2, 2, 2> BK 64) + split-K 2
H_, W_ = 62, 64     # 3 968 pixels as one 62 x 64 sample


def _record(case, ratio, x=None):
    U.record_parity("numeric_edges/" + case, round(ratio, 4))
    if x is not None:
        U.record_parity("numeric_edges/" + case + "@x", x)
    assert ratio <= 1.0, (case, ratio)


def _last_launch(lib):
    info = (ctypes.c_int * 4)()
    assert lib.ladi_igemm_last_launch(info) == 0
    return dict(family=FAMILY.get(info[0], info[0]), split=info[2])


def _template_args(lib, cfg):
    sym = lib.ladi_igemm_cfg_symbol_name(cfg).decode()
    return sym.split("<")[0], [int(v) for v in sym.split("<")[1].rstrip(">").split(",")]


def _igemm(lib, X, C, W, B, Q, act, cfg, ldo, P=NE.PIX, hw=(H_, W_), stats=None, ln=None, gn=None):
    """one ladi_op_igemm(_stats) launch of a 1 x 1 problem on the guarded operand X into a fresh guarded output; returns (rc, out, px)"""
    Qout = Q // 2 if act == "geglu" else Q
    out = U.guarded_out(P, Qout, ld=ldo, pre_rows=4, post_rows=4)
    d = _lib.IGemmDesc()
    d.src0, d.C0, d.ld0 = X.ptr, C, X.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = hw[0], hw[1], hw[0], hw[1], P
    d.ksize, d.stride, d.pad, d.ups = 1, 1, 0, 0
    d.W, d.Q, d.K, d.ldw = W.data_ptr(), Q, C, 0
    d.bias, d.act, d.out_scale = (B.data_ptr() if B is not None else None), U.ACT[act], 1.0
    keep = []
    if ln is not None:
        gm, bt = ln[0].half().to(U.dev()), ln[1].half().to(U.dev())
        keep += [gm, bt]
        d.ln_gamma, d.ln_beta, d.ln_eps = gm.data_ptr(), bt.data_ptr(), float(ln[2])
        if ln[3]:
            scr = torch.empty((P, C), dtype=torch.float16, device=U.dev())
            keep.append(scr)
            d.ln_scratch = scr.data_ptr()
    if gn is not None:
        d.gn_ss, d.gn_hw = gn[0].data_ptr(), int(gn[1])
    d.out, d.ldo = out.ptr, ldo
    px = ctypes.c_int(0)
    if stats is not None:
        d.stats = stats.ptr
        rc = lib.ladi_op_igemm_stats(ctypes.byref(d), 1, cfg, ctypes.byref(px), stream_ptr())
    else:
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
    torch.cuda.synchronize()
    return rc, out, px.value


# ---------------------------------------------------------------------------------------------------------------------- A. sweep operands
@functools.lru_cache(maxsize=None)
def _sweep_x(C):
    return U.guarded(NE.sweep_operand(C), ld=C + 64, pre_rows=4, post_rows=4)


@functools.lru_cache(maxsize=None)
def _sweep_w(K, geglu=False):
    if geglu:
        w, b = NE.geglu_interleave(*NE.geglu_operands(K))
        return w.half().contiguous().to(U.dev()), b.half().to(U.dev())
    return NE.selection_weight(K).half().contiguous().to(U.dev()), None


def _judge_sweep(case, out, ref, bound, inputs, x=None, out_f32=False, locate=NE.locate_point):
    got = out.cpu().float() if not out_f32 else out.cpu()
    U.check_elem(got, ref, bound, case, locate, out_f32=out_f32)
    U.assert_untouched(out, case + " output")
    for g in inputs:
        U.assert_untouched(g, case + " input")
    ratio, xw = NE.worst_point(got, ref, bound, NE.sweep()["x"] if x is None else x, out_f32=out_f32)
    _record(case, ratio, xw)


def _sweep_case(lib, case, act, cfg, ldo, C=128, stats=False, family="ring", split=1):
    geglu = act == "geglu"
    X = _sweep_x(C)
    W, B = _sweep_w(C, geglu)
    Q = 2 * NE.CH if geglu else NE.CH
    st = S.poisoned_rows(NE.PIX, NE.CH) if stats else None
    rc, out, px = _igemm(lib, X, C, W, B, Q, act, cfg, ldo, stats=st)
    assert rc == 0, "%s: cfg %d refused the launch: rc = %d (%s)" % (case, cfg, rc, _lib.last_error())
    info = _last_launch(lib)
    assert info["family"] == family and info["split"] == split, (case, info)
    ref, bound = NE.geglu_sweep_ref(C) if geglu else NE.sweep_ref(act)
    _judge_sweep(case, out, ref, bound, [X])
    return out, px


def _fast_epilogue(out, ldo):
    """igemm_epilogue's dispatch condition for these launches (no residual, no batch, Qout = 64)"""
    return ldo % 8 == 0 and out.ptr % 16 == 0


# 1 / 3: the two epilogues of the tiled kernels, non-GEGLU.  ldo = 72: fp16 rows of whole 16-byte chunks -> igemm_epilogue_fast (silu_fast, gelu_f);
# ldo = 68 (ld % 8 == 4) -> igemm_epilogue_generic (silu_f, gelu_f)
@pytest.mark.parametrize("act", ["silu", "gelu", "relu"])
@pytest.mark.parametrize("epilogue,ldo", [("fast", 72), ("generic", 68)])
def test_igemm_epilogue_activation_sweep(lib, epilogue, ldo, act):
    name, targs = _template_args(lib, RING)
    assert name == "igemm_kernel"
    out, _ = _sweep_case(lib, "epilogue_%s/%s" % (epilogue, act), act, RING, ldo)
    assert _fast_epilogue(out, ldo) == (epilogue == "fast")


# 2 / 4: GEGLU through igemm_epilogue_fast<..., true> and through the generic routine's own branch
@pytest.mark.parametrize("epilogue,ldo", [("fast", 72), ("generic", 68)])
def test_igemm_epilogue_geglu_sweep(lib, epilogue, ldo):
    name, targs = _template_args(lib, RING)
    assert name == "igemm_kernel" and targs[2] % 2 == 0          # TQ even: the fast GEGLU epilogue exists for this tile
    out, _ = _sweep_case(lib, "epilogue_%s/geglu" % epilogue, "geglu", RING, ldo)
    assert _fast_epilogue(out, ldo) == (epilogue == "fast")


def test_geglu_is_refused_on_tiles_with_odd_tq(lib):
    """igemm_epilogue would route GEGLU on an odd-TQ tile to the generic routine, whose last u block has no g block: the table marks those
    configurations as not GEGLU-capable and the launcher refuses (-8) -- the generic GEGLU branch is reached by alignment only (above)"""
    name, targs = _template_args(lib, RING_ODD_TQ)
    assert name == "igemm_kernel" and targs[2] % 2 == 1
    W, B = _sweep_w(128, True)
    rc, out, _ = _igemm(lib, _sweep_x(128), 128, W, B, 128, "geglu", RING_ODD_TQ, 72)
    assert rc == -8, rc
    assert bool(torch.isnan(out.cpu()).all())


# 5 / 6: split-K.  K = 256 in two slices: the non-zero weights (channels 0..127) sit in the first, the second contributes exact zeros.  The
# statistics-row height the launch reports tells the forms apart: 32 = splitk_reduce_kernel, 32 TP = the in-launch combine + fused epilogue
@pytest.mark.parametrize("form,act", [("two_pass", "silu"), ("two_pass", "gelu"), ("in_launch", "silu")])
def test_split_k_activation_sweep(lib, form, act):
    name, targs = _template_args(lib, SPLITK)
    assert name == "igemm_kernel"
    try:
        lib.ladi_igemm_set_splitk_two_pass(1 if form == "two_pass" else 0)
        _, px = _sweep_case(lib, "splitk_%s/%s" % (form, act), act, SPLITK, 72, C=256, stats=True, split=2)
    finally:
        lib.ladi_igemm_set_splitk_two_pass(0)
    assert px == (32 if form == "two_pass" else 32 * targs[3]), (form, px)


# 7: linear_xs MODE 2
@pytest.mark.parametrize("cfg", [25, 93])
def test_linear_xs_geglu_sweep(lib, cfg):
    _sweep_case(lib, "linear_xs_geglu/cfg%d" % cfg, "geglu", cfg, 72, C=320, family="linear_xs")


# 8: small_linear_kernel -- one-hot weights with K = 8: out[m][n] = act(x[m][n]), the fp16 sweep alone
@pytest.mark.parametrize("act,pre", [("silu", 0), ("gelu", 0), ("relu", 0), ("tanh", 0), ("none", 1)])
def test_small_linear_activation_sweep(lib, act, pre):
    x = NE.finite_halves().reshape(-1, 8)
    M = x.shape[0]
    gx, gw = U.guarded(x, ld=16), U.guarded(torch.eye(8).half())
    go = U.guarded_out(M, 8, ld=16)
    rc = lib.ladi_op_small_linear(gx.ptr, 0, gx.ld, gw.ptr, None, None, 0, M, 8, 8, U.ACT[act], pre, go.ptr, 0, go.ld, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ref, bound = NE.sweep_ref_halves(act, bool(pre))
    case = "small_linear/" + ("pre_silu" if pre else act)
    _judge_sweep(case, go, ref, bound, [gx, gw], x=x.double(), locate=lambda i: "x = %r" % float(x.reshape(-1)[i]))


# 9: the fp32 path -- the halves widened to fp32, identity weights, fp32 stores (where the reference is exactly 0 -- ReLU of a negative -- so
# must the output be: U32 |ref| leaves no room).  ReLU and tanh only, the two the warping path uses with this sweep's range: act_f32's SiLU
# has results far below the fp32 normal range here (1e-305 at -65504), which a relative fp32 bound cannot judge
def _judge_f32(case, go, act, inputs):
    x = NE.finite_halves().double().reshape(-1, 8)
    ref, bound = NE.sweep_ref_halves(act)
    got = go.cpu()
    zero = ref == 0
    assert bool((got[zero] == 0).all()), case
    for g in inputs + [go]:
        U.assert_untouched(g, case)
    U.check_elem(got[~zero], ref[~zero], bound[~zero], case, out_f32=True)
    ratio, xw = NE.worst_point(got[~zero], ref[~zero], bound[~zero], x[~zero], out_f32=True)
    _record(case, ratio, xw)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_conv_f32_activation_sweep(lib, act):
    x = NE.finite_halves().float().reshape(-1, 8)
    P = x.shape[0]
    g0, gw, go = U.guarded(x, ld=12), U.guarded(torch.eye(8)), U.guarded_out(P, 8, ld=12, dtype=torch.float32)
    d = ConvF32Desc()
    d.src0, d.C0, d.ld0 = g0.ptr, 8, g0.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = P // 64, 64, P // 64, 64, P
    d.ksize, d.stride, d.pad = 1, 1, 0
    d.W, d.Q, d.K, d.ldw = gw.ptr, 8, 8, 0
    d.act, d.out, d.ldo = U.ACT[act], go.ptr, go.ld
    rc = lib.ladi_op_conv_f32(ctypes.byref(d), 1, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _judge_f32("conv_f32/" + act, go, act, [g0, gw])


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_linear_f32_activation_sweep(lib, act):
    x = NE.finite_halves().float().reshape(-1, 8)
    M = x.shape[0]
    gx, gw, go = U.guarded(x, ld=12), U.guarded(torch.eye(8)), U.guarded_out(M, 8, ld=12, dtype=torch.float32)
    rc = lib.ladi_op_linear_f32(ctypes.c_void_p(gx.ptr), gx.ld, ctypes.c_void_p(gw.ptr), None, M, 8, 8, U.ACT[act], ctypes.c_void_p(go.ptr), go.ld, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _judge_f32("linear_f32/" + act, go, act, [gx, gw])


# 10: GroupNorm + SiLU (silu_fast in gn_norm_kernel and in gn_apply_kernel) at arguments of about +-1700
def _group_norm(lib, x, c0, c1, n, HW, gamma, beta, eps, silu):
    dense = lambda t: U.guarded(t.half().contiguous(), pre_rows=8, post_rows=8)
    X0, X1 = dense(x[:, :c0]), (dense(x[:, c0:]) if c1 else None)
    G, B = gamma.half().to(U.dev()), beta.half().to(U.dev())
    out = U.guarded_out(n * HW, c0 + c1, pre_rows=8, post_rows=8)
    rc = lib.ladi_op_group_norm(X0.ptr, c0, X1.ptr if c1 else None, c1, n, HW, NE.GROUPS, ptr(G), ptr(B), eps, silu, None, out.ptr, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    return out, [g for g in (X0, X1) if g is not None]


@pytest.mark.parametrize("onepass", ["1", "0"])
def test_group_norm_silu_at_large_arguments(lib, monkeypatch, onepass):
    monkeypatch.setenv("LADI_GN_ONEPASS", onepass)
    c = NE.gn_silu_case()
    out, inputs = _group_norm(lib, c["x"], c["C"], 0, c["n"], c["HW"], c["gamma"], c["beta"], 1e-5, 1)
    case = "group_norm_silu/onepass%s" % onepass
    _judge_sweep(case, out, c["ref"], c["bound"], inputs, x=c["pre"], locate=U.pixel_locator(c["n"], c["HW"], 1, c["C"]))


# ---------------------------------------------------------------------------------------------------------------------- B. norms
def _runs():
    """(family, eps): the eps-dominated family with both values; constant and zero inputs cannot tell them apart and run with both all the same"""
    return [(k, e) for k in NE.FAMILIES for e in NE.EPS_VALUES]


def _judge_norm(case, kind, out, ref, bound, beta, inputs, silu=0, locate=None):
    got = out.cpu().float()
    ratio = U.check_elem(got, ref, bound, case, locate)
    U.assert_untouched(out, case + " output")
    for g in inputs:
        U.assert_untouched(g, case + " input")
    if kind == "zero" and not silu:
        assert torch.equal(out.cpu(), beta.half()[None, :].expand(got.shape[0], -1)), case + ": an all-zero input must give exactly fp16(beta)"
    _record(case, ratio)


@pytest.mark.parametrize("kind,eps", _runs())
@pytest.mark.parametrize("name,c0,c1,HW", NE.GN_SHAPES)
@pytest.mark.parametrize("onepass", ["1", "0"])
def test_group_norm_where_eps_decides(lib, monkeypatch, onepass, name, c0, c1, HW, kind, eps):
    """ladi_op_group_norm: LADI_GN_ONEPASS=1 gn_norm_kernel (HW = 48: its direct-statistics branch), =0 gn_partial + gn_finalize + gn_apply"""
    monkeypatch.setenv("LADI_GN_ONEPASS", onepass)
    for silu in (0, 1):
        x, gamma, beta, ref, bound = NE.gn_case(kind, c0, c1, HW, eps, silu)
        out, inputs = _group_norm(lib, x, c0, c1, 2, HW, gamma, beta, eps, silu)
        _judge_norm("group_norm/%s-onepass%s-%s-eps%g-silu%d" % (name, onepass, kind, eps, silu), kind, out, ref, bound, beta, inputs, silu,
                    U.pixel_locator(2, HW, 1, c0 + c1))


@pytest.mark.parametrize("kind,eps", _runs())
@pytest.mark.parametrize("HW,px", NE.GN_ROWS)
def test_group_norm_rows_where_eps_decides(lib, HW, px, kind, eps):
    """ladi_op_group_norm_rows on producer-shaped rows: rps = 3 and 96 (gn_norm_kernel), 97 (gn_reduce_rows_kernel first)"""
    x, gamma, beta, ref, bound = NE.gn_case(kind, 64, 0, HW, eps, 0)
    X = U.guarded(x.half(), pre_rows=8, post_rows=8)
    rows = S.rows_buffer(S.block_rows(x, 2, HW, px), 4)
    G, B = gamma.half().to(U.dev()), beta.half().to(U.dev())
    out = U.guarded_out(2 * HW, 64, pre_rows=8, post_rows=8)
    rc = lib.ladi_op_group_norm_rows(X.ptr, 64, rows.ptr, px, None, 0, None, 0, 2, HW, NE.GROUPS, ptr(G), ptr(B), eps, 0, None, out.ptr, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    _judge_norm("group_norm_rows/rps%d-%s-eps%g" % (HW // px, kind, eps), kind, out, ref, bound, beta, [X, rows], 0, U.pixel_locator(2, HW, 1, 64))


@pytest.mark.parametrize("kind,eps", _runs())
@pytest.mark.parametrize("C,rows", NE.LN_SHAPES)
def test_layer_norm_where_eps_decides(lib, C, rows, kind, eps):
    """ladi_op_layer_norm_ld, the five layernorm_kernel instantiations"""
    x, gamma, beta, ref, bound = NE.ln_case(kind, rows, C, eps)
    X = U.guarded(x.half(), ld=C + 8, pre_rows=4, post_rows=4)
    G, B = gamma.half().to(U.dev()), beta.half().to(U.dev())
    out = U.guarded_out(rows, C, ld=C + 16, pre_rows=4, post_rows=4)
    assert lib.ladi_op_layer_norm_ld(X.ptr, X.ld, ptr(G), ptr(B), eps, rows, C, out.ptr, out.ld, stream_ptr()) == 0
    torch.cuda.synchronize()
    _judge_norm("layer_norm/C%d-rows%d-%s-eps%g" % (C, rows, kind, eps), kind, out, ref, bound, beta, [X], 0, lambda i: "(row, c) = (%d, %d)" % (i // C, i % C))


@pytest.mark.parametrize("kind,eps", [("eps", 1e-5), ("eps", 1e-6), ("zero", 1e-6)])
@pytest.mark.parametrize("route,cfg", [("fused", 25), ("fused", 93), ("scratch", 7)])
def test_linear_behind_layer_norm_where_eps_decides(lib, route, cfg, kind, eps):
    """LayerNorm fused into linear_xs's prologue, and the stand-alone kernel through the caller's scratch in front of a tiled kernel"""
    x, gamma, beta, w, b, ref, bound = NE.ln_linear_case(kind, eps)
    P = x.shape[0]
    X = U.guarded(x.half(), ld=NE.XS_C + 64, pre_rows=4, post_rows=4)
    W, B = w.half().contiguous().to(U.dev()), b.half().to(U.dev())
    rc, out, _ = _igemm(lib, X, NE.XS_C, W, B, NE.XS_Q, "none", cfg, NE.XS_Q + 8, P=P, hw=(NE.XS_H, NE.XS_W), ln=(gamma, beta, eps, route == "scratch"))
    assert rc == 0, _lib.last_error()
    assert _last_launch(lib)["family"] == ("linear_xs" if route == "fused" else "ring")
    case = "linear_layer_norm/%s-cfg%d-%s-eps%g" % (route, cfg, kind, eps)
    ratio = U.check_elem(out.cpu().float(), ref, bound, case, U.pixel_locator(1, NE.XS_H, NE.XS_W, NE.XS_Q))
    U.assert_untouched(out, case + " output")
    U.assert_untouched(X, case + " input")
    _record(case, ratio)


@pytest.mark.parametrize("kind,eps", [("eps", 1e-5), ("eps", 1e-6), ("zero", 1e-6)])
def test_linear_behind_group_norm_affine_where_eps_decides(lib, kind, eps):
    """the GroupNorm affine folded into linear_xs's register panel, scale / shift from statistics with this eps (scale ~ 200-300)"""
    x, ss, w, b, ref, bound = NE.gn_linear_case(kind, eps)
    P = x.shape[0]
    X = U.guarded(x.half(), ld=NE.XS_C + 64, pre_rows=4, post_rows=4)
    W, B, SS = w.half().contiguous().to(U.dev()), b.half().to(U.dev()), ss.to(U.dev())
    rc, out, _ = _igemm(lib, X, NE.XS_C, W, B, NE.XS_Q, "none", 25, NE.XS_Q + 8, P=P, hw=(2 * NE.XS_H, NE.XS_W), gn=(SS, NE.XS_H * NE.XS_W))
    assert rc == 0, _lib.last_error()
    assert _last_launch(lib)["family"] == "linear_xs"
    case = "linear_group_norm/%s-eps%g" % (kind, eps)
    ratio = U.check_elem(out.cpu().float(), ref, bound, case, U.pixel_locator(2, NE.XS_H, NE.XS_W, NE.XS_Q))
    U.assert_untouched(out, case + " output")
    U.assert_untouched(X, case + " input")
    _record(case, ratio)


@pytest.mark.parametrize("C", [8, 512, 520])
def test_l2norm_rows_f16_where_eps_decides(lib, C):
    x = NE.l2norm_rows(C, 2800 + C, True)
    ref, bound = HC.l2norm_ref_bound(x)
    gx, gy = U.guarded(x.half(), ld=C + 8), U.guarded_out(5, C, ld=C + 16)
    assert lib.ladi_op_l2norm_rows(gx.ptr, gx.ld, 5, C, gy.ptr, gy.ld, stream_ptr()) == 0
    torch.cuda.synchronize()
    U.assert_untouched(gx, "input")
    U.assert_untouched(gy, "output")
    got = gy.cpu()
    assert not bool(got[4].any()), "the zero row must come out as zeros"
    _record("l2norm/C%d" % C, U.check_elem(got, ref, bound, "l2norm_rows C = %d" % C))


@pytest.mark.parametrize("C", [8, 72, 512])
def test_l2norm_rows_f32_where_eps_decides(lib, C):
    x = NE.l2norm_rows(C, 2800 + C, False)
    ref, bound = HC.l2norm_ref_bound(x)
    gx = U.guarded(x, ld=C + 4)
    assert lib.ladi_op_l2norm_rows_f32(ctypes.c_void_p(gx.ptr), gx.ld, 5, C, stream_ptr()) == 0
    torch.cuda.synchronize()
    U.assert_untouched(gx, "operand")
    got = gx.cpu()
    assert not bool(got[4].any()), "the zero row must stay zero"
    _record("l2norm_f32/C%d" % C, U.check_elem(got[:4], ref[:4], bound[:4], "l2norm_rows_f32 C = %d" % C, out_f32=True))


def test_fused_cross_attention_block_where_eps_decides(lib):
    c = NE.xattn_case(1e-6)
    d = lambda t: t.half().contiguous().to(U.dev())
    X, KV, G, B, WQ, WO, BO = d(c["x"]), d(c["kv"]), d(c["gamma"]), d(c["beta"]), d(c["wq"]), d(c["wo"]), d(c["bo"])
    out = torch.empty_like(X)
    rc = lib.ladi_op_xattn_block(ptr(X), ptr(G), ptr(B), 1e-6, ptr(WQ), ptr(KV), c["L"], ptr(WO), ptr(BO), c["n"], c["T"], ptr(out), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    err = U.rel_l2(out.float().cpu(), c["ref"])
    U.record_parity("numeric_edges/xattn_block/eps1e-06", round(err / NE.XF_TOL, 4))
    assert err < NE.XF_TOL, err


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_fused_feed_forward_block_where_eps_decides(lib, monkeypatch, pipe):
    monkeypatch.setenv("LADI_FF_PIPE", pipe)
    c = NE.ff_case(1e-6)
    d = lambda t: t.half().contiguous().to(U.dev())
    X, G, B, W1, B1, W2, BO = d(c["x"]), d(c["gamma"]), d(c["beta"]), d(c["w1"]), d(c["b1"]), d(c["w2"]), d(c["bo"])
    out = torch.empty_like(X)
    rc = lib.ladi_op_ff_block(ptr(X), ptr(G), ptr(B), 1e-6, ptr(W1), ptr(B1), ptr(W2), ptr(BO), c["P"], ptr(out), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    err = U.rel_l2(out.float().cpu(), c["ref"])
    U.record_parity("numeric_edges/ff_block/pipe%s-eps1e-06" % pipe, round(err / NE.XF_TOL, 4))
    assert err < NE.XF_TOL, err


# ---------------------------------------------------------------------------------------------------------------------- D. the VAE's eps s^2
@pytest.mark.parametrize("shift", [0, NE.VAE_SHIFT])
def test_vae_decode_rescales_eps_with_the_range_shift(shift):
    """the tiny VAE with its residual stream scaled by 2^-VAE_K, where an eps that is not multiplied by s^2 at shift 4 costs the oracle 20 dB
    (tests/test_cpu_numeric_edges.py): the native decoder at range shift 0 and 4 against the oracle on the same state dict"""
    import ladi_vton_amd as L
    from oracle import models as M
    vcfg, sd0, z = NE.vae_tiny()
    sd = NE.vae_scaled_state_dict(sd0, NE.VAE_K)
    ref = M.vae_decode(sd, vcfg, z)
    vae = L.NativeVAE(vcfg, sd)
    vae.range_shift = shift
    out = vae.decode(z.to(U.dev())).sample.float().cpu()
    torch.cuda.synchronize()
    assert vae.last_range_shift == shift
    db = U.psnr(out, ref)
    U.record_parity("numeric_edges/vae_eps_rescale/shift%d_psnr_db" % shift, round(db, 2))
    assert db >= NE.VAE_PSNR_DB, (shift, db)
