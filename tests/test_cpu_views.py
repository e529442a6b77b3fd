"""The guarded-view harness of tests/util.py judged on its own, without a GPU: torch's fp32 conv2d / layer_norm / softmax @ V, rounded to
fp16, pass the per-element check against float64 at the shapes tests/test_gpu_views.py runs; the same outputs with one element moved by
three fp16 ulps, or one border pixel scaled by 0.9, are rejected; assert_untouched fires on a single flipped poison element."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import util as U


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def _rejects(got, ref, bound, what):
    with pytest.raises(AssertionError):
        U.check_elem(got, ref, bound, what)


def _perturbations_rejected(got, ref, bound, border, what):
    """got (fp16-rounded values of a passing result) with (a) the element whose bound is tightest in ulps moved by 3 ulps, (b) the slice
    `border` scaled by 0.9"""
    ulp = U.ulp16(ref)
    tight = bound / ulp
    i = int(tight.reshape(-1).argmin())
    # 3 ulps minus the half ulp (and the fp32 error) the clean result may already be off must still exceed ulp + bound
    assert float(tight.reshape(-1)[i]) < 1.4, (what, float(tight.min()))
    moved = got.clone().double()
    flat = moved.reshape(-1)
    away = 1.0 if float(flat[i]) >= float(ref.reshape(-1)[i]) else -1.0
    flat[i] += away * 3.0 * float(ulp.reshape(-1)[i])
    _rejects(moved, ref, bound, what + " +3ulp")
    scaled = got.clone().double()
    scaled[border] *= 0.9
    _rejects(scaled, ref, bound, what + " border x0.9")


@pytest.mark.parametrize("N,c0,c1,cout,h,w,act,res", [(3, 128, 0, 320, 20, 13, "none", True), (3, 128, 64, 320, 20, 13, "silu", True),
                                                      (2, 64, 0, 3, 16, 12, "none", False), (2, 128, 0, 128, 16, 64, "silu", False)])
def test_check_elem_accepts_torch_conv_and_rejects_perturbations(N, c0, c1, cout, h, w, act, res):
    cin = c0 + c1
    x, wt, b = _rand((N, cin, h, w), 70), _rand((cout, cin, 3, 3), 71, 1 / math.sqrt(9 * cin)), _rand((cout,), 72, 0.1)
    r = _rand((N, cout, h, w), 73) if res else None
    ref, bound = U.conv_ref_bound(x, wt, bias=b, act=act, res=r)
    y = F.conv2d(x, wt, b, padding=1)
    y = {"none": lambda v: v, "silu": F.silu}[act](y)
    got = ((y.half().float() + r) if res else y).half()      # the library's rounding points (conv_ref_bound's docstring)
    worst = U.check_elem(got.float(), ref, bound, "conv")
    assert worst <= 1.0
    _perturbations_rejected(got.float(), ref, bound, (0, slice(None), 0, 0), "conv")
    _perturbations_rejected(got.float(), ref, bound, (N - 1, slice(None), h - 1, w - 1), "conv")


@pytest.mark.parametrize("rows,C", [(77, 512), (4097, 520), (4097, 1536), (77, 1544), (5, 4096)])
def test_check_elem_accepts_torch_layer_norm_and_rejects_perturbations(rows, C):
    x, g, b = _rand((rows, C), 36, 3.0) + 1, _rand((C,), 37, 0.1) + 1, _rand((C,), 38, 0.1)
    ref, bound = U.layer_norm_ref_bound(x, g, b, 1e-5)
    got = F.layer_norm(x, (C,), g, b, 1e-5).half().float()
    assert U.check_elem(got, ref, bound, "layer_norm") <= 1.0
    _perturbations_rejected(got, ref, bound, (rows - 1, slice(None)), "layer_norm")


@pytest.mark.parametrize("n,heads,Nq,Nk", [(2, 2, 192, 192), (1, 5, 300, 77), (1, 2, 33, 130)])
def test_check_elem_accepts_torch_attention_and_rejects_perturbations(n, heads, Nq, Nk):
    def heads_of(t):
        return t.view(n, -1, heads, 64).transpose(1, 2)
    # (a) the inputs of the GPU tests: accepted; a border query row scaled by 0.9 is rejected
    q, k, v = (heads_of(_rand((n, N_, heads * 64), s)) for N_, s in ((Nq, 40), (Nk, 41), (Nk, 42)))
    ref, bound = U.attention_ref_bound(q, k, v, 0.125)
    got = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).half().float()
    assert U.check_elem(got, ref, bound, "attention") <= 1.0
    scaled = got.clone()
    scaled[n - 1, heads - 1, Nq - 1] *= 0.9
    _rejects(scaled, ref, bound, "attention border x0.9")
    # (b) the bound charges the kernel's fp16 rounding of the pre-scaled query and of the probabilities, worst case over all keys: with
    # logits of a few units that is tens of ulps.  Small logits and a positive V (sum p |v| = |ref|) bring it under 1.4 ulps, where
    # a 3-ulp move of one element must be caught as well
    q, k = q * 0.1, k * 0.1
    v = v.abs() + 0.5
    ref, bound = U.attention_ref_bound(q, k, v, 0.125)
    got = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).half().float()
    assert U.check_elem(got, ref, bound, "attention") <= 1.0
    _perturbations_rejected(got, ref, bound, (0, 0, 0), "attention")


def test_check_elem_fails_on_a_non_finite_element():
    ref = torch.ones((4, 8), dtype=torch.float64)
    got = torch.ones((4, 8))
    assert U.check_elem(got, ref, 0.0, "ones") == 0.0
    got[2, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        U.check_elem(got, ref, 1e30, "ones")
    got[2, 3] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        U.check_elem(got, ref, 1e30, "ones")


def test_ulp16():
    x = torch.tensor([1.0, 1.999, 2.0, 0.75, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9], dtype=torch.float64)
    assert torch.equal(U.ulp16(x), want)
    # agrees with the spacing of torch's own fp16 numbers
    h = torch.tensor([0.1, 1.5, 300.0, 6.0e-6], dtype=torch.float16)
    nxt = (h.view(torch.int16) + 1).view(torch.float16)
    assert torch.equal(U.ulp16(h.double()), nxt.double() - h.double())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_guarded_layout_and_assert_untouched(dtype):
    t = torch.arange(5 * 24, dtype=torch.float32).reshape(5, 24).to(dtype)
    g = U.guarded(t, ld=32, pre_rows=3, post_rows=2, device="cpu")
    assert g.ld == 32 and g.rows == 5 and g.C == 24 and g.ptr % 16 == 0 and g.ptr == g.buf.data_ptr() + 3 * 32 * t.element_size()
    assert torch.equal(g.cpu(), t)
    full = g.buf.reshape(10, 32)
    assert bool(torch.isnan(full[:3]).all()) and bool(torch.isnan(full[8:]).all()) and bool(torch.isnan(full[3:8, 24:]).all())
    assert int(g.poison_mask().sum()) == 10 * 32 - 5 * 24
    U.assert_untouched(g)
    g.view[2, 5] = 123.0                   # writing INSIDE the view is the kernel's job
    U.assert_untouched(g)
    # a single flipped poison element, at each kind of place: the row before, the padding columns of a row, the row after
    it = torch.int16 if dtype == torch.float16 else torch.int32
    for r, c in ((2, 31), (4, 24), (8, 0)):
        g2 = U.guarded(t, ld=32, pre_rows=3, post_rows=2, device="cpu")
        bits = g2.buf.view(it).reshape(10, 32)
        bits[r, c] ^= 1                    # still a NaN: only the raw pattern differs
        assert bool(torch.isnan(g2.buf.reshape(10, 32)[r, c]))
        with pytest.raises(AssertionError, match="allocation row %d .*column %d" % (r, c)):
            U.assert_untouched(g2, "flip")
    # an NHWC operand is flattened to pixel rows; a dense one (ld = C) keeps only the poison rows
    g3 = U.guarded(torch.zeros((2, 3, 4, 8), dtype=dtype), device="cpu")
    assert g3.rows == 24 and g3.ld == 8 and int(g3.poison_mask().sum()) == 4 * 8
    out = U.guarded_out(6, 8, ld=16, device="cpu", dtype=dtype)
    assert bool(torch.isnan(out.buf).all())


# ---------------------------------------------------------------------------------------------------------------------- far views
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("samples,sstride", [(1, None), (3, None), (3, 5 * 1000 + 7 * 8)])
def test_far_view_harness_places_detects_strays_and_unwritten_elements(dtype, samples, sstride, monkeypatch):
    """guarded_far() / assert_untouched_far() at a small span on the CPU, with the chunk size cut down so that the allocation takes several
    chunks: (1) every operand element sits where the documented formula says and everything else is poison, (2) ONE planted stray write is
    found wherever it lies -- the first and last element of the allocation, the column behind a row, the gap between two samples, a chunk
    boundary --, (3) an output element that was never written fails check_elem, a fully written output passes and leaves the count at zero."""
    monkeypatch.setattr(U, "FAR_CHUNK", 1000)
    srows, C, ld = 4, 24, 1000
    t = (_rand((samples * srows, C), 5) if dtype == torch.float16 else _rand((samples * srows, C), 5)).to(dtype)
    g = U.guarded_far(t, ld, samples=samples, sstride=sstride, device="cpu")
    ss = srows * ld if sstride is None else sstride
    it, word = U._poison_word(dtype)
    bits = g.buf.view(it)
    assert g.buf.numel() == 2 * U.FAR_PAD + (samples - 1) * ss + (srows - 1) * ld + C and g.buf.numel() > 3 * U.FAR_CHUNK
    expect = torch.full_like(bits, word)
    for s in range(samples):
        for r in range(srows):
            e0 = U.FAR_PAD + s * ss + r * ld
            assert torch.equal(g.buf[e0:e0 + C], t[s * srows + r])
            expect[e0:e0 + C] = t[s * srows + r].view(it)
    assert torch.equal(bits, expect)
    assert torch.equal(g.cpu(), t) and g.ptr == g.buf.data_ptr() + U.FAR_PAD * g.buf.element_size()
    assert g.last_byte == ((samples - 1) * ss + (srows - 1) * ld + C) * g.buf.element_size() - 1
    U.assert_untouched_far(g, "clean")
    spots = [0, g.buf.numel() - 1, U.FAR_PAD - 1, U.FAR_PAD + C, U.FAR_PAD + ld - 1, U.FAR_PAD + (srows - 1) * ld + C, 2 * U.FAR_CHUNK - 1, 2 * U.FAR_CHUNK]
    if samples > 1:
        spots += [U.FAR_PAD + ss - 1, U.FAR_PAD + (samples - 1) * ss + C]
    inside = g.inside(torch.tensor(spots))
    assert not bool(inside.any()), (spots, inside)
    assert bool(g.inside(torch.tensor([U.FAR_PAD, U.FAR_PAD + C - 1, U.FAR_PAD + (samples - 1) * ss + (srows - 1) * ld + C - 1])).all())
    for e in spots:
        keep = bits[e].clone()
        g.buf[e] = 0.0
        assert U.far_stray_count(g) == 1, e
        with pytest.raises(AssertionError, match="allocation elements %d " % e):
            U.assert_untouched_far(g, "stray at %d" % e)
        bits[e] = keep
    U.assert_untouched_far(g, "restored")
    # an operand element that changes is no stray (a kernel may write its output), whatever it holds
    g.views[-1][srows - 1, C - 1] = 3.0
    U.assert_untouched_far(g, "operand write")
    out = U.guarded_far_out(samples * srows, C, ld, samples=samples, sstride=sstride, dtype=dtype, device="cpu")
    for s, v in enumerate(out.views):
        v.copy_(t[s * srows:(s + 1) * srows])
    assert U.check_elem(out.cpu().float(), t.double(), 0.0, "written") == 0.0
    U.assert_untouched_far(out, "written output")
    out.views[samples - 1][srows - 1, C - 1] = float("nan")          # as an element the launch never reached
    _rejects(out.cpu().float(), t.double(), 0.0, "unwritten")
