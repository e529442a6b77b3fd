"""Operator-level checks of the helper kernels and of the fp32 warping path (csrc/elementwise.hip, f32path.hip, attention.hip
attn_single_query_kernel), each through its own ladi_op_* entry point.

Conventions (tests/util.py): every operand is a guarded() view -- ld > C wherever the launcher takes a stride, NaN rows before and after --
and assert_untouched() runs on every operand and on the output after the launch.  Kernels that move data or round once are compared with
torch.equal against the CPU result; accumulating kernels with check_elem against the float64 references and derived bounds of
tests/helpers_cases.py.  Every case records its worst err / limit under helpers/... in the parity file and must end with a ratio <= 1."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ConvF32Desc, stream_ptr
from tests import helpers_cases as HC
from tests import util as U

pytestmark = pytest.mark.gpu

F32, F16 = _lib.F32, _lib.F16
f32, f16 = torch.float32, torch.float16

# Relative error of the kernel's own frequencies exp(-ln(10000) j / half) -- __expf and the fp32 arithmetic of its argument -- in fp32 ulps.  No
# ROCm document on the build machine states the accuracy of __expf, so the figure is measured: test_timestep_embedding recovers the frequencies
# from a t = 1 launch and writes the largest relative error against math.exp to the parity file as helpers/timestep_expf_ulps.  Measured on
# an MI355X: 12.674 units of 2^-24 over dim 320 and 1280 (most of it the fp32 rounding of the argument -ln(10000) j / half, up to 9.2, before
# the exponential sees it).  The bound grants TWICE the measured value, as a stated allowance and nothing more.
EXPF_ULPS_MEASURED = 12.674
EXPF_ULPS_GRANTED = None if EXPF_ULPS_MEASURED is None else 2.0 * EXPF_ULPS_MEASURED


def P(x):
    return ctypes.c_void_p(x.ptr if isinstance(x, U.Guarded) else x)


def sync():
    torch.cuda.synchronize()


def untouched(*gs):
    for i, g in enumerate(gs):
        U.assert_untouched(g, "operand %d" % i)


def flatg(t, out=False):
    """a dense buffer (any shape) as ONE guarded row between poison rows"""
    t2 = t.reshape(1, -1)
    if out:
        return U.guarded_out(1, t2.shape[1], dtype=t.dtype, any_ld=True)
    return U.guarded(t2, any_ld=True)


def record(key, ratio):
    U.record_parity("helpers/" + key, ratio)
    assert ratio <= 1.0, (key, ratio)


INT_POISON = 0x5A5A5A5A


class IntBuf:
    """int32 operand or output between 16 poison words on either side"""

    def __init__(self, t=None, n=None):
        n = t.numel() if t is not None else n
        self.n = n
        self.buf = torch.full((n + 32,), INT_POISON, dtype=torch.int32, device=U.dev())
        if t is not None:
            self.buf[16:16 + n] = t.reshape(-1).to(U.dev())
        self.ptr = self.buf.data_ptr() + 64

    def cpu(self):
        return self.buf[16:16 + self.n].cpu()

    def check(self):
        b = self.buf.cpu()
        assert bool((b[:16] == INT_POISON).all()) and bool((b[16 + self.n:] == INT_POISON).all()), "poison around an int buffer was overwritten"


# ------------------------------------------------------------------------------------------------------------ single-query attention
@pytest.mark.parametrize("case", HC.SQ_CASES, ids=lambda c: "d%d_h%d_k%d_n%d_q%g" % c)
def test_attention_single_query(lib, case):
    d, heads, Nk, n, _ = case
    q, kv, scale, ref, bound = HC.single_query_case(*case)
    H = heads * d
    gq = U.guarded(q.half(), ld=H + 8)
    gkv = U.guarded(kv.half().reshape(n * Nk, 2 * H))            # k | v interleaved: row stride 2 H, v at column H, samples Nk rows apart
    go = U.guarded_out(n, H, ld=H + 8)
    rc = lib.ladi_op_attention_single_query(P(gq), gq.ld, P(gkv), 2 * H, ctypes.c_void_p(gkv.col(H)), 2 * H, P(go), go.ld, n, heads, d, Nk,
                                            Nk * 2 * H, Nk * 2 * H, scale, stream_ptr())
    assert rc == 0, rc
    sync()
    untouched(gq, gkv, go)
    record("single_query/d%d_h%d_k%d_n%d_q%g" % case, U.check_elem(go.cpu(), ref, bound, "single query %r" % (case,),
                                                                  lambda i: "(sample %d, head %d, lane %d)" % (i // H, i % H // d, i % d)))


def test_attention_single_query_refuses_a_head_wider_than_two_lanes(lib):
    go = U.guarded_out(1, 136)
    g = U.guarded(torch.zeros((4, 272), dtype=f16))
    assert lib.ladi_op_attention_single_query(P(g), 272, P(g), 272, P(g), 272, P(go), 136, 1, 1, 129, 2, 0, 0, 1.0, stream_ptr()) == -1
    sync()
    untouched(go)


# ----------------------------------------------------------------------------------------------------------------------- small_linear
def _small_linear(lib, x, xf, w, b, res, M, N, K, act, pre, of, ldx=None):
    gx = U.guarded(x if xf else x.half(), ld=(K + 8 if ldx is None else ldx))
    gw, gb = U.guarded(w.half()), U.guarded(b.half().reshape(1, -1), any_ld=True)
    gr = U.guarded(res.half(), ld=N + 8, any_ld=True) if res is not None else None       # N + 8 = 58, 109: scalar loads and stores
    go = U.guarded_out(M, N, ld=N + 8, dtype=f32 if of else f16, any_ld=True)
    rc = lib.ladi_op_small_linear(P(gx), int(xf), gx.ld, P(gw), P(gb), P(gr) if gr else None, gr.ld if gr else 0, M, N, K, U.ACT[act], int(pre),
                                  P(go), int(of), go.ld, stream_ptr())
    sync()
    untouched(*[g for g in (gx, gw, gb, gr, go) if g is not None])
    return rc, go


@pytest.mark.parametrize("case", HC.SL_CASES, ids=lambda c: "_".join(str(v) for v in c))
def test_small_linear(lib, case):
    xf, of, act, pre, has_res, M, N, K = case
    x, w, b, res, ref, bound = HC.small_linear_case(*case)
    rc, go = _small_linear(lib, x, xf, w, b, res, M, N, K, act, pre, of)
    assert rc == 0, rc
    record("small_linear/" + "_".join(str(v) for v in case),
           U.check_elem(go.cpu(), ref, bound, "small_linear %r" % (case,), lambda i: "(row %d, column %d)" % (i // N, i % N), out_f32=bool(of)))


def test_small_linear_refuses_unaligned_k_and_stride(lib):
    x, w, b = torch.zeros((2, 16)), torch.zeros((4, 16)), torch.zeros(4)
    rc, go = _small_linear(lib, x[:, :12], 0, w[:, :12], b, None, 2, 4, 12, "none", 0, 0, ldx=16)      # K % 8 != 0
    assert rc == -1 and bool(torch.isnan(go.cpu()).all())
    rc, go = _small_linear(lib, x, 0, w, b, None, 2, 4, 16, "none", 0, 0, ldx=20)                      # ldx % 8 != 0
    assert rc == -1 and bool(torch.isnan(go.cpu()).all())


@pytest.mark.parametrize("K", [768, 40])
def test_linear_f32(lib, K):
    M, N = 2, 50
    x, w, b, ref, bound = HC.linear_f32_case(K)
    gx, gw, gb, go = U.guarded(x, ld=K + 4), U.guarded(w), U.guarded(b.reshape(1, -1), any_ld=True), U.guarded_out(M, N, ld=N + 2, dtype=f32, any_ld=True)
    assert lib.ladi_op_linear_f32(P(gx), gx.ld, P(gw), P(gb), M, N, K, U.ACT["tanh"], P(go), go.ld, stream_ptr()) == 0
    sync()
    untouched(gx, gw, gb, go)
    record("linear_f32/K%d" % K, U.check_elem(go.cpu(), ref, bound, "linear_f32 K = %d" % K, out_f32=True))


# --------------------------------------------------------------------------------------------------------------------------- conv_f32
def _conv_desc(c, g0, g1, gw, gb, go):
    d = ConvF32Desc()
    d.src0, d.C0, d.ld0 = g0.ptr, c.C0, g0.ld
    if g1 is not None:
        d.src1, d.C1, d.ld1 = g1.ptr, c.C1, g1.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = c.H, c.W, c.Ho, c.Wo, c.P
    d.ksize, d.stride, d.pad = c.k, c.stride, c.pad
    d.W, d.Q, d.K, d.ldw = gw.ptr, c.Q, c.K, 0
    d.bias = gb.ptr if gb is not None else None
    d.act, d.out, d.ldo = U.ACT[c.act], go.ptr, go.ld
    return d


def _conv_operands(c):
    g0 = U.guarded(c.src0, ld=c.ld0)
    g1 = U.guarded(c.src1, ld=c.ld1) if c.src1 is not None else None
    gw = U.guarded(c.w)
    gb = U.guarded(c.bias.reshape(1, -1), any_ld=True) if c.bias is not None else None
    go = U.guarded_out(c.P, c.Q, ld=c.ldo, dtype=f32, any_ld=True)
    return g0, g1, gw, gb, go


@pytest.mark.parametrize("name", ["a3", "a8", "b", "c", "d", "f"])
def test_conv_f32(lib, name):
    c = HC.conv_f32_cases()[name]
    ops = _conv_operands(c)
    d = _conv_desc(c, *ops)
    rc = lib.ladi_op_conv_f32(ctypes.byref(d), 1, stream_ptr())
    assert rc == 0, rc
    sync()
    untouched(*[g for g in ops if g is not None])
    bp, bq = (256, 64) if c.Q <= 64 else (128, 128)
    record("conv_f32/" + name, U.check_elem(ops[-1].cpu(), c.ref, c.bound, "conv_f32 case " + name,
                                            U.pixel_locator(c.N, c.Ho, c.Wo, c.Q, bq, bp), out_f32=True))


def _corr_desc(gb_, ga, go, B, C, hw):
    d = ConvF32Desc()
    d.src0, d.C0, d.ld0 = gb_.ptr, C, gb_.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = 6, 4, 6, 4, hw
    d.ksize, d.stride, d.pad = 1, 1, 0
    d.W, d.Q, d.K, d.ldw = ga.ptr, hw, C, C
    d.bs_src0, d.bs_w, d.bs_out = hw * gb_.ld, hw * C, hw * go.ld
    d.act, d.out, d.ldo = 0, go.ptr, go.ld
    return d


def test_conv_f32_batched_correlation(lib):
    """case e: the launch of the TPS correlation -- batch 2, the weight operand a feature map at ldw = C, every operand a batch stride"""
    B, C, hw = 2, 16, 24
    fb, fa, ref, bound = HC.conv_f32_corr_case()
    gb_, ga, go = U.guarded(fb.reshape(B * hw, C), ld=20), U.guarded(fa.reshape(B * hw, C)), U.guarded_out(B * hw, hw, ld=32, dtype=f32)
    d = _corr_desc(gb_, ga, go, B, C, hw)
    rc = lib.ladi_op_conv_f32(ctypes.byref(d), B, stream_ptr())
    assert rc == 0, rc
    sync()
    untouched(gb_, ga, go)
    record("conv_f32/e", U.check_elem(go.cpu().reshape(B, hw, hw), ref, bound, "conv_f32 case e", out_f32=True))


def test_conv_f32_refuses_bad_arguments_without_a_launch(lib):
    """rc -1 / -3 / -4 existed before this test; -5 (ld < C), -6 (batch > 1 with a second source) and -7 (batch strides off 16 bytes) were
    added with it -- those launches used to run"""
    c = HC.conv_f32_cases()["b"]
    ops = _conv_operands(c)
    g0, g1, gw, gb, go = ops

    def run(batch=1, **kw):
        d = _conv_desc(c, *ops)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ladi_op_conv_f32(ctypes.byref(d), batch, stream_ptr())

    assert run(C0=12, K=9 * 28) == -1                          # existing: channels not a multiple of 8
    assert run(ld0=10) == -1                                   # existing: row stride not a multiple of 4
    assert run(K=c.K + 8) == -3                                # existing: K != ksize^2 (C0 + C1)
    assert run(ldw=6) == -3                                    # existing: weight row stride not a multiple of 4
    assert run(src0=g0.ptr + 4) == -4                          # existing: a source 4 bytes off the 16-byte boundary
    assert run(ld0=4) == -5                                    # new: ld0 < C0 = 8
    assert run(ld1=8) == -5                                    # new: ld1 < C1 = 16
    assert run(batch=2) == -6                                  # new: batch > 1 with src1 / C1
    one = dict(src1=None, C1=0, ld1=0, K=9 * 8, ldw=c.K)       # the single-source form of the same operands, for the batch strides
    assert run(batch=2, bs_src0=6, **one) == -7                # new
    assert run(batch=2, bs_w=c.K + 2, **one) == -7             # new
    assert run(batch=2, bs_out=go.ld + 1, **one) == -7         # new (ldo = 72: the vector store)
    sync()
    untouched(*ops)
    assert bool(torch.isnan(go.cpu()).all())


# ----------------------------------------------------------------------------------------------------------------------- fp32 helpers
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_nchw_nhwc_f32_round_trip(lib, half):
    n, C, H, W, ld = 2, 21, 4, 7, 24
    x = HC.randn((n, C, H, W), 1600, half=half)
    gs = flatg(x.half() if half else x)
    gd = U.guarded_out(n * H * W, ld, dtype=f32)              # the kernel writes all ld columns: zeros at and above C
    assert lib.ladi_op_nchw_to_nhwc_f32(P(gs), F16 if half else F32, n, C, H, W, P(gd), ld, stream_ptr()) == 0
    sync()
    untouched(gs, gd)
    want = torch.zeros((n, H, W, ld))
    want[..., :C] = x.permute(0, 2, 3, 1)
    assert torch.equal(gd.cpu(), want.reshape(-1, ld))
    gsrc = U.guarded(want.reshape(-1, ld)[:, :C], ld=ld)      # back: columns [C, ld) are poison and must not be read
    for dt, code in ((f32, F32), (f16, F16)):
        gb = flatg(torch.empty((n, C, H, W), dtype=dt), out=True)
        assert lib.ladi_op_nhwc_to_nchw_f32(P(gsrc), ld, n, C, H, W, P(gb), code, stream_ptr()) == 0
        sync()
        untouched(gsrc, gb)
        assert torch.equal(gb.cpu().reshape(n, C, H, W), x.to(dt))


def test_channel_affine_f32(lib):
    """x * scale[c] + shift[c] is ONE fused multiply-add in fp32: the only error is the rounding check_elem(out_f32) grants (bound 0)"""
    n_pix, C, ld = 37, 24, 28
    x, sc, sh = HC.randn((n_pix, C), 1610), HC.randn((C,), 1611), HC.randn((C,), 1612)
    gx, gs, gh = U.guarded(x, ld=ld), flatg(sc), flatg(sh)
    assert lib.ladi_op_channel_affine_f32(P(gx), ld, n_pix, C, P(gs), P(gh), stream_ptr()) == 0
    sync()
    untouched(gx, gs, gh)
    record("channel_affine_f32", U.check_elem(gx.cpu(), x.double() * sc.double() + sh.double(), 0.0, "channel_affine_f32", out_f32=True))


@pytest.mark.parametrize("C", [8, 72, 512])
def test_l2norm_rows_f32(lib, C):
    x = HC.l2norm_input(C, 1500 + C, False)
    ref, bound = HC.l2norm_ref_bound(x)
    gx = U.guarded(x, ld=C + 4)
    assert lib.ladi_op_l2norm_rows_f32(P(gx), gx.ld, 5, C, stream_ptr()) == 0
    sync()
    untouched(gx)
    got = gx.cpu()
    assert not bool(got[3].any()), "the zero row must stay zero"
    live = [0, 1, 2, 4]                                        # the zero row has reference and bound 0: judged by the equality above
    record("l2norm_f32/C%d" % C, U.check_elem(got[live], ref[live], bound[live], "l2norm_rows_f32 C = %d" % C, out_f32=True))


GATHER_IDX = [5, 0, 5, 3, 6, 1, 0, 2]          # duplicates and a permutation


def test_gather_rows_f32_and_f16(lib):
    H = 40
    idx = IntBuf(torch.tensor(GATHER_IDX, dtype=torch.int32))
    for dt, fn in ((f32, lib.ladi_op_gather_rows_f32), (f16, lib.ladi_op_gather_rows)):
        src = HC.randn((7, H), 1620, half=True).to(dt)
        gs, gd = U.guarded(src), U.guarded_out(len(GATHER_IDX), H, dtype=dt)
        assert fn(P(gs), ctypes.c_void_p(idx.ptr), len(GATHER_IDX), H, P(gd), stream_ptr()) == 0
        sync()
        untouched(gs, gd)
        idx.check()
        assert torch.equal(gd.cpu(), src[GATHER_IDX])


def test_maxpool2_f32(lib):
    n, C, H, W, ld = 2, 8, 10, 6, 12
    x = HC.randn((n, C, H, W), 1630)
    gs, gd = U.guarded(x.permute(0, 2, 3, 1), ld=ld), U.guarded_out(n * (H // 2) * (W // 2), C, ld=ld, dtype=f32)
    assert lib.ladi_op_maxpool2_f32(P(gs), ld, n, H, W, C, P(gd), ld, stream_ptr()) == 0
    sync()
    untouched(gs, gd)
    assert torch.equal(gd.cpu(), F.max_pool2d(x, 2).permute(0, 2, 3, 1).reshape(-1, C))
    assert lib.ladi_op_maxpool2_f32(P(gs), ld, n, 5, 12, C, P(gd), ld, stream_ptr()) == -1        # odd height


@pytest.mark.parametrize("shape", [(2, 8, 10, 6), (1, 8, 1, 1), (1, 8, 1, 4)], ids=["10x6", "1x1", "1x4"])
def test_upsample2x_bilinear_f32(lib, shape):
    n, C, H, W = shape
    x = HC.randn(shape, 1520 + W)
    ref, bound = HC.upsample_ref_bound(x)
    gs, gd = U.guarded(x.permute(0, 2, 3, 1), ld=12), U.guarded_out(n * 4 * H * W, C, ld=12, dtype=f32)
    assert lib.ladi_op_upsample2x_bilinear_f32(P(gs), 12, n, H, W, C, P(gd), 12, stream_ptr()) == 0
    sync()
    untouched(gs, gd)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    record("upsample_f32/%dx%d" % (H, W), U.check_elem(gd.cpu(), nhwc(ref), nhwc(bound.expand_as(ref)), "upsample2x f32 %dx%d" % (H, W),
                                                         U.pixel_locator(n, 2 * H, 2 * W, C), out_f32=True))


# ------------------------------------------------------------------------------------------------------------------- fp16 TPS helpers
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_channel_affine_f16(lib, in_place):
    """(h16)(x * scale + shift): one fp32 fused multiply-add, u |ref|, then the fp16 rounding"""
    n_pix, C = 37, 24
    x, sc, sh = HC.randn((n_pix, C), 1640, half=True), HC.randn((C,), 1641), HC.randn((C,), 1642)
    gx, gs, gh = U.guarded(x.half(), ld=32), flatg(sc), flatg(sh)
    gy = gx if in_place else U.guarded_out(n_pix, C, ld=40)
    assert lib.ladi_op_channel_affine(P(gx), gx.ld, n_pix, C, P(gs), P(gh), P(gy), gy.ld, stream_ptr()) == 0
    sync()
    untouched(gx, gs, gh, gy)
    if not in_place:
        assert torch.equal(gx.cpu(), x.half())
    ref = x.double() * sc.double() + sh.double()
    record("channel_affine/" + ("in_place" if in_place else "out_of_place"), U.check_elem(gy.cpu(), ref, U.U32 * ref.abs(), "channel_affine"))


@pytest.mark.parametrize("C", [8, 512, 520])
def test_l2norm_rows_f16(lib, C):
    x = HC.l2norm_input(C, 1510 + C, True)
    ref, bound = HC.l2norm_ref_bound(x)
    gx, gy = U.guarded(x.half(), ld=C + 8), U.guarded_out(5, C, ld=C + 16)
    assert lib.ladi_op_l2norm_rows(P(gx), gx.ld, 5, C, P(gy), gy.ld, stream_ptr()) == 0
    sync()
    untouched(gx, gy)
    got = gy.cpu()
    assert not bool(got[3].any()), "the zero row must come out as zeros"
    record("l2norm/C%d" % C, U.check_elem(got, ref, bound, "l2norm_rows C = %d" % C))        # ulp16 keeps the zero row's limit positive


@pytest.mark.parametrize("case", HC.TPS_CASES, ids=lambda c: "N%d_%dx%d" % c)
def test_tps_grid(lib, case):
    N, H, W = case
    coor, inv, ctrl, ref, bound = HC.tps_case(*case)
    gc, gi, gt, go = flatg(coor), flatg(inv), flatg(ctrl), flatg(torch.empty((2, H, W, 2)), out=True)
    assert lib.ladi_op_tps_grid(P(gc), P(gi), P(gt), N, 2, H, W, P(go), stream_ptr()) == 0
    sync()
    untouched(gc, gi, gt, go)
    record("tps_grid/N%d_%dx%d" % case, U.check_elem(go.cpu().reshape(2, H, W, 2), ref, bound, "tps_grid %r" % (case,),
                                                      lambda i: "(b, y, x, xy) = (%d, %d, %d, %d)" % (i // (2 * H * W), i // (2 * W) % H, i // 2 % W, i % 2),
                                                      out_f32=True))


def test_tps_grid_refuses_too_many_points_and_a_one_pixel_axis(lib):
    z = flatg(torch.zeros(36 * 36))
    go = flatg(torch.empty((2, 4, 4, 2)), out=True)
    assert lib.ladi_op_tps_grid(P(z), P(z), P(z), 33, 2, 4, 4, P(go), stream_ptr()) == -1
    assert lib.ladi_op_tps_grid(P(z), P(z), P(z), 4, 2, 16, 1, P(go), stream_ptr()) == -1
    sync()
    untouched(go)


# -------------------------------------------------------------------------------------------------------------------- text and vision
@pytest.mark.parametrize("use_words", [1, 0])
def test_text_meta(lib, use_words):
    ids = HC.text_meta_ids()
    B, T = ids.shape
    gi, gf, ge = IntBuf(ids), IntBuf(n=B), IntBuf(n=B)
    assert lib.ladi_op_text_meta(ctypes.c_void_p(gi.ptr), B, T, HC.TEXT_VSTAR, use_words, ctypes.c_void_p(gf.ptr), ctypes.c_void_p(ge.ptr), stream_ptr()) == 0
    sync()
    for g in (gi, gf, ge):
        g.check()
    first, eot = HC.text_meta_ref(ids, HC.TEXT_VSTAR, use_words)
    assert gf.cpu().tolist() == first.tolist()
    assert ge.cpu().tolist() == eot.tolist() == (torch.arange(B) * T + ids.argmax(1)).tolist()


@pytest.mark.parametrize("H", [8, 1024])
@pytest.mark.parametrize("with_words", [True, False], ids=["wemb", "null"])
def test_text_embed(lib, H, with_words):
    B, T, vocab, nv = 2, 77, 320, 4
    ids = torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(1700), dtype=torch.int32)
    ids[0, 5], ids[1, 9], ids[0, 76] = -5, 400, 400            # clamped to rows 0 and 319
    first = torch.tensor([75, -1], dtype=torch.int32)          # the window of sentence 0 runs past its end; sentence 1 has none
    tok, pos, wemb = HC.randn((vocab, H), 1701, half=True).half(), HC.randn((T, H), 1702, half=True).half(), HC.randn((B, nv, H), 1703, half=True).half()
    gi, gf = IntBuf(ids), IntBuf(first)
    gt, gp, gw, go = U.guarded(tok), U.guarded(pos), U.guarded(wemb.reshape(B * nv, H)), U.guarded_out(B * T, H)
    rc = lib.ladi_op_text_embed(ctypes.c_void_p(gi.ptr), ctypes.c_void_p(gf.ptr), nv, P(gt), P(gp), P(gw) if with_words else None, B, T, H, vocab,
                                P(go), stream_ptr())
    assert rc == 0, rc
    sync()
    untouched(gt, gp, gw, go)
    gi.check()
    gf.check()
    want = HC.text_embed_ref(ids, first, nv, tok, pos, wemb if with_words else None)
    assert torch.equal(go.cpu().view(torch.int16), want.reshape(B * T, H).view(torch.int16))
    assert torch.equal(want[0, 5], (tok[0].float() + pos[5].float()).half()) and torch.equal(want[1, 9], (tok[319].float() + pos[9].float()).half())


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_patchify(lib, half):
    B, S, ps, KP = 2, 28, 14, 640
    px = HC.randn((B, 3, S, S), 1710, half=half)
    gs, go = flatg(px.half() if half else px), U.guarded_out(B * 5, KP)
    assert lib.ladi_op_patchify(P(gs), F16 if half else F32, B, S, ps, KP, P(go), stream_ptr()) == 0
    sync()
    untouched(gs, go)
    got, want = go.cpu().reshape(B, 5, KP), HC.patchify_ref(px, ps, KP)
    assert torch.equal(got, want)
    assert not bool(got[:, 0].any()) and not bool(got[:, :, 588:].any())


# -------------------------------------------------------------------------------------------------------------------------- loop glue
def _timestep(lib, t, dim):
    gt, go = flatg(torch.tensor(t, dtype=f32)), U.guarded_out(len(t), dim, dtype=f32)
    assert lib.ladi_op_timestep_embedding(P(gt), len(t), dim, P(go), stream_ptr()) == 0
    sync()
    untouched(gt, go)
    return go.cpu()


def test_timestep_embedding(lib):
    """measures the relative error of the kernel's frequencies first (EXPF_ULPS_* above): with t = 1 the outputs are cos f_j and sin f_j, and
    atan2(sin, cos) returns f_j, well conditioned for every j (f_j in [1e-4, 1]: sin f_j carries f_j's relative error where f_j is small, cos f_j
    where it is not); the 2 ulps of cosf / sinf themselves are part of the measured figure"""
    worst = 0.0
    for dim in (320, 1280):
        half = dim // 2
        o = _timestep(lib, [1.0], dim).double()[0]
        f = torch.atan2(o[half:], o[:half])
        worst = max(worst, float(((f - HC.timestep_freq(dim)).abs() / HC.timestep_freq(dim)).max()) / U.U32)
    print("helpers/timestep_expf_ulps = %.3f" % worst)
    U.record_parity("helpers/timestep_expf_ulps", worst)
    assert EXPF_ULPS_GRANTED is not None, "measured %.3f fp32 ulps; EXPF_ULPS_MEASURED is not set" % worst
    for dim in (320, 1280):                                     # 1280: blockIdx.y > 0 of the launcher's tiling of the half dimension
        ref, bound = HC.timestep_ref_bound(HC.TIMESTEPS, dim, EXPF_ULPS_GRANTED)
        got = _timestep(lib, HC.TIMESTEPS, dim)
        ratio = U.check_elem(got, ref, bound, "timestep_embedding dim %d" % dim, lambda i: "(t = %g, column %d)" % (HC.TIMESTEPS[i // dim], i % dim),
                             out_f32=True)
        print("helpers/timestep/dim%d = %.3f" % (dim, ratio))
        record("timestep/dim%d" % dim, ratio)


def test_image_post_over_every_finite_half(lib):
    x = HC.all_finite_halves()
    n = x.shape[0]
    want_f, want_u = HC.image_post_ref(x)
    gs = U.guarded(x, ld=8)
    gf = U.guarded_out(n, 3, dtype=f32, any_ld=True)
    assert lib.ladi_op_image_post(P(gs), 8, n, P(gf), 0, stream_ptr()) == 0
    u8 = torch.full((n * 3 + 64,), 0xA5, dtype=torch.uint8, device=U.dev())
    assert lib.ladi_op_image_post(P(gs), 8, n, ctypes.c_void_p(u8.data_ptr() + 32), 1, stream_ptr()) == 0
    sync()
    untouched(gs, gf)
    assert torch.equal(gf.cpu(), want_f)
    u8 = u8.cpu()
    assert bool((u8[:32] == 0xA5).all()) and bool((u8[32 + 3 * n:] == 0xA5).all())
    assert torch.equal(u8[32:32 + 3 * n].reshape(n, 3), want_u)


@pytest.mark.parametrize("with_pq", [True, False], ids=["pq", "identity"])
def test_post_quant(lib, with_pq):
    n, ld, inv_sf = 37, 64, 1.0 / 0.18215
    lat, pq = HC.randn((n, 4), 1530, 4.0), HC.randn((20,), 1531, 0.5)
    ref, bound = HC.post_quant_ref_bound(lat, pq if with_pq else None, inv_sf)
    gl, gp, go = U.guarded(lat), flatg(pq), U.guarded_out(n, ld)          # every column of a row is written: zeros from channel 4 on
    assert lib.ladi_op_post_quant(P(gl), P(gp) if with_pq else None, inv_sf, n, P(go), ld, stream_ptr()) == 0
    sync()
    untouched(gl, gp, go)
    got = go.cpu()
    assert not bool(got[:, 4:].any()) and bool(torch.isfinite(got).all())
    record("post_quant/" + ("pq" if with_pq else "identity"), U.check_elem(got[:, :4], ref, bound, "post_quant"))


def test_latents_layout_round_trip(lib):
    B, hw = 2, 35
    x = HC.randn((B, 4, hw), 1720)
    gs, gp, gb = flatg(x), U.guarded_out(B * hw, 4, dtype=f32), flatg(torch.empty_like(x), out=True)
    assert lib.ladi_op_lat_nchw_to_pix(P(gs), B, hw, 1.0, P(gp), stream_ptr()) == 0
    assert lib.ladi_op_lat_pix_to_nchw(P(gp), B, hw, P(gb), stream_ptr()) == 0
    sync()
    untouched(gs, gp, gb)
    assert torch.equal(gp.cpu().reshape(B, hw, 4), x.permute(0, 2, 1))
    assert torch.equal(gb.cpu().reshape(B, 4, hw), x)


@pytest.mark.parametrize("cfg", [0, 1])
def test_latents_import(lib, cfg):
    B, hw, ld_in, s = 2, 35, 64, 0.7
    x = HC.randn((B, 4, hw), 1730)
    rows = (2 if cfg else 1) * B * hw
    gs, gl, gu = flatg(x), U.guarded_out(B * hw, 4, dtype=f32), U.guarded_out(rows, 4, ld=ld_in)      # channels 4..63 of unet_in are poison
    assert lib.ladi_op_latents_import(P(gs), B, hw, P(gl), P(gu), ld_in, cfg, s, stream_ptr()) == 0
    sync()
    untouched(gs, gl, gu)
    pix = x.permute(0, 2, 1).reshape(B * hw, 4)
    assert torch.equal(gl.cpu(), pix)
    want = (pix * torch.tensor(s, dtype=f32)).half()
    assert torch.equal(gu.cpu().view(torch.int16), (torch.cat([want, want]) if cfg else want).view(torch.int16))
    assert lib.ladi_op_latents_import(P(gs), B, hw, P(gl), P(gu), 6, cfg, s, stream_ptr()) == -1


def test_scale_h16(lib):
    n_pix, C, s = 37, 72, 0.3
    x = HC.randn((n_pix, C), 1740, 8.0, half=True).half()
    gs, gd = U.guarded(x, ld=80), U.guarded_out(n_pix, C, ld=96)
    assert lib.ladi_op_scale_h16(P(gs), 80, P(gd), 96, n_pix, C, s, stream_ptr()) == 0
    sync()
    untouched(gs, gd)
    assert torch.equal(gd.cpu().view(torch.int16), (x.float() * torch.tensor(s, dtype=f32)).half().view(torch.int16))


@pytest.mark.parametrize("n", [1, 70001])
def test_fill_f32(lib, n):
    g = flatg(torch.empty(n), out=True)
    assert lib.ladi_op_fill_f32(P(g), n, 1.5, stream_ptr()) == 0
    sync()
    untouched(g)
    assert torch.equal(g.cpu().reshape(-1), torch.full((n,), 1.5))
