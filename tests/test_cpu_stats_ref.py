"""The reference side of tests/test_gpu_stats.py, checked without a GPU: the bound of tests/util.py stats_rows_ref_bound holds for fp32
emulations of three summation orders, and tests/stats_cases.py judge_rows -- the function that judges every producer on the GPU -- accepts a
faithful CPU producer and rejects each planted defect."""
import pytest
import torch

from tests import stats_cases as S
from tests import util as U


def _sequential(t):
    """fp32 sum over dim 0, one term after the other"""
    acc = torch.zeros_like(t[0])
    for row in t:
        acc = acc + row
    return acc


def _pairwise(t):
    """fp32 tree sum over dim 0: halves added until one row is left (an odd row is carried)"""
    while t.shape[0] > 1:
        m = t.shape[0] // 2
        head = t[:m] + t[m:2 * m]
        t = torch.cat([head, t[2 * m:]]) if t.shape[0] % 2 else head
    return t[0]


def _lanes_then_tree(t, lanes=64):
    """64 lanes, each summing every 64th term in order, then a tree over the lanes: the shape of a wave-wide reduction"""
    part = torch.stack([_sequential(t[l::lanes]) if t[l::lanes].shape[0] else torch.zeros_like(t[0]) for l in range(lanes)])
    return _pairwise(part)


ORDERS = dict(sequential=_sequential, pairwise=_pairwise, lanes_then_tree=_lanes_then_tree)


def _values(kind):
    if kind == "epilogue":                       # the stored output of the emulated producer: 384 pixels per sample, half of them masked
        p = S.emulated_producer()
        return p.stored, p.n, p.HW
    if kind == "positive":                       # all of one sign: nothing cancels, the running sum grows past every term's binade
        return (S.rand((2 * 3072, 16), 790).abs() + 0.25).half().double(), 2, 3072
    if kind == "vae":                            # 6144 pixels per sample, all of one sign (a reduced VAE level of tests/test_gpu_tuned.py): above
        return (S.rand((2 * 6144, 8), 792).abs() + 0.25).half().double(), 2, 6144      # 4096 the helper grants gamma_(HW - 1) itself
    return S.rand((2 * 4096, 8), 791, 30.0).double(), 2, 4096          # the largest HW for which HW u stands in for gamma_(HW - 1), large values


@pytest.mark.parametrize("kind", ["epilogue", "positive", "wide", "vae"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_bound_holds_for_fp32_summation_orders(order, kind):
    stored, n, HW = _values(kind)
    ssum, ssq, bsum, bsq = U.stats_rows_ref_bound(stored, n, HW)
    v = stored.float().reshape(n, HW, -1)
    assert bool((v.double() == stored.reshape(n, HW, -1)).all())
    for s in range(n):
        got_sum, got_sq = ORDERS[order](v[s]), ORDERS[order](v[s] * v[s])
        assert got_sum.dtype == torch.float32
        e1, e2 = (got_sum.double() - ssum[s]).abs(), (got_sq.double() - ssq[s]).abs()
        assert bool((e1 <= bsum[s]).all()), (order, kind, s, float((e1 / bsum[s]).max()))
        assert bool((e2 <= bsq[s]).all()), (order, kind, s, float((e2 / bsq[s]).max()))


def test_bound_is_tight_enough_to_see_one_missing_pixel():
    """dropping ONE pixel of a sample moves the sum of squares of most channels by more than the bound"""
    p = S.emulated_producer()
    ssum, ssq, bsum, bsq = U.stats_rows_ref_bound(p.stored, p.n, p.HW)
    px = int(p.stored[:p.HW].abs().sum(1).argmax())
    drop = p.stored[px] ** 2
    assert int((drop > bsq[0]).sum()) > p.Q // 2, int((drop > bsq[0]).sum())


def test_judge_on_samples_above_4096_pixels():
    """HW = 6144 in rows of 256 pixels (the gamma branch of stats_rows_ref_bound): faithful rows pass; a row credited to the other sample, a
    block of pixels counted twice and one missing pixel fail"""
    stored, n, HW = _values("vae")
    px = 256
    rows = S.block_rows(stored, n, HW, px)
    cap = (n * HW + 31) // 32
    assert S.judge_rows(S.rows_buffer(rows, 4, device="cpu", cap=cap), px, stored, n, HW, "faithful") < 1.0
    rps = HW // px
    swapped = rows.clone()
    swapped[[rps - 1, rps]] = rows[[rps, rps - 1]]
    doubled = rows.clone()
    doubled[3] = rows[3] + S.block_rows(stored[3 * px:3 * px + 32], 1, 32, 32)[0]
    missing = rows.clone()
    missing[rps + 1] = S.block_rows(torch.cat([stored[(rps + 1) * px:(rps + 2) * px - 1], torch.zeros(1, stored.shape[1]).double()]), 1, px, px)[0]
    for name, bad in (("row in the other sample", swapped), ("32 pixels twice", doubled), ("one pixel missing", missing)):
        with pytest.raises(AssertionError):
            S.judge_rows(S.rows_buffer(bad, 4, device="cpu", cap=cap), px, stored, n, HW, name)


def test_judge_accepts_the_faithful_producer():
    p = S.emulated_producer()
    ratio = S.judge_rows(p.rows(), p.px, p.stored, p.n, p.HW, "faithful")
    assert ratio < 1.0


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_judge_rejects_planted_defects(defect):
    """(a) one row moved to the other sample, (b) the last 8-channel octet of the Q = 96 problem left as poison, (c) statistics taken before
    the residual add, (d) before the mask, and a row of zeros written behind the last one"""
    p = S.emulated_producer()
    with pytest.raises(AssertionError):
        S.judge_rows(p.rows(defect), p.px, p.stored, p.n, p.HW, defect)


def test_judge_rejects_a_touched_guard_row_and_a_wrong_row_height():
    p = S.emulated_producer()
    g = p.rows()
    g.buf[0] = 0.0
    with pytest.raises(AssertionError):
        S.judge_rows(g, p.px, p.stored, p.n, p.HW, "guard row")
    with pytest.raises(AssertionError):                     # rows of 128 pixels read as rows of 64: half of them were never written
        S.judge_rows(p.rows(), 64, p.stored, p.n, p.HW, "row height")
    with pytest.raises(AssertionError):
        S.assert_all_poison(p.rows(), "demoted")
    S.assert_all_poison(S.poisoned_rows(768, 96, device="cpu"), "untouched")


def test_expected_row_px_follows_the_symbol():
    assert S.expected_row_px("igemm_kernel<2, 2, 2, 4, 32, 3, 2, 0>", 1, False, 384) == 128
    assert S.expected_row_px("igemm_kernel<2, 2, 5, 3, 64, 2, 1, 1>", 1, False, 256) == 0          # 256 pixels are no whole rows of 96
    assert S.expected_row_px("igemm8_kernel<5, 2, 0>", 2, False, 384) == 64 and S.expected_row_px("igemm8_kernel<5, 2, 0>", 2, True, 384) == 32
    assert S.expected_row_px("igemm_lc_kernel<2, 2, 2, 2, 2, 4>", 2, False, 384) == 32
    assert S.expected_row_px("igemm_halo_kernel<2, 3, 1, 3, 2, 24, 0, 0, 0>", 1, False, 384) == 96
    assert S.expected_row_px("linear_xs_kernel", 1, False, 384) == 0


def test_synthetic_rows_add_up_to_the_source():
    c = S.consumer_case(64, 0, 384)
    for px in (384, 128, 96, 32):
        rows = c.rows(0, px)
        assert rows.shape == (2 * 384 // px, 64, 2) and rows.dtype == torch.float32
        g = S.rows_buffer(rows, 4, device="cpu")
        assert S.judge_rows(g, px, c.source(0).double(), 2, 384, "synthetic px %d" % px) < 1.0
