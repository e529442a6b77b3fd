"""The judges of tests/test_gpu_numeric_edges.py, checked without a GPU (tests/numeric_edge_cases.py holds the data).

Activation sweep: the sweep's pre-activations are exact in fp32; fp32 emulations of the three formulas of csrc/common.h pass the judge over the
whole fp16 domain, and each planted mistake (tanh-approximation GELU, x sigmoid(1.702 x), SiLU where GELU is asked) is rejected at thousands of
points -- most of them beyond what N(0, 1) pre-activations reach.
Norms: every eps-dominated case can tell eps = 1e-5 from 1e-6 and from none at all (the float64 reference with the other eps lies outside the
limit at >= 90 % of the elements), and an fp32 one-pass emulation with the right eps passes."""
import numpy as np
import pytest
import torch

from tests import helpers_cases as HC
from tests import numeric_edge_cases as NE
from tests import util as U

MIN_DISCRIMINATION = 0.90


# ---------------------------------------------------------------------------------------------------------------------- the sweep itself
def test_sweep_covers_every_finite_half_and_is_exact_in_fp32():
    s = NE.sweep()
    h = NE.finite_halves()
    assert h.numel() == 63488 and bool(torch.isfinite(h).all()) and s["x"].numel() == 253952
    assert torch.equal(s["a"].reshape(-1, 4)[:, 0].half().view(torch.int16), h.view(torch.int16))      # every bit pattern, +-0 and subnormals included
    # both operands are halves, both products are exact in fp32 and so is their sum in either order: at most 14 significant bits
    a32, c32 = s["a"].float(), s["c"].float()
    assert bool((a32.double() == s["a"]).all()) and bool((c32.half().float() == c32).all())
    p1, p2 = a32 * 1.0, c32 * np.float32(NE.W2)
    assert bool((p2.double() == s["c"] * NE.W2).all())
    assert bool(((p1 + p2).double() == s["x"]).all()) and bool(((p2 + p1).double() == s["x"]).all())
    mant = s["x"] / torch.exp2(torch.floor(torch.log2(s["x"].abs().clamp_min(2.0 ** -40))) - 13)
    assert bool((mant == mant.round()).all())
    # j = 1..3 are quarter-ulp steps away from zero, strictly between the half and its neighbour
    step = (s["x"] - s["a"]).abs() / U.ulp16(s["a"])
    top = s["a"].abs() >= 32768
    assert bool((step[~top].reshape(-1, 4) == torch.tensor([0.0, 0.25, 0.5, 0.75], dtype=torch.float64)).all())
    assert bool((step[top].reshape(-1, 4) == torch.tensor([0.0, 0.25, 0.25, 0.25], dtype=torch.float64)).all())
    assert int(s["sub"].sum()) == 4 * 2048
    # every reference is finite in fp16
    for act in ("silu", "gelu", "relu", "tanh"):
        assert bool(torch.isfinite(NE.sweep_ref(act)[0].half()).all()), act
    assert bool(torch.isfinite(NE.geglu_sweep_ref()[0].half()).all())


def test_gelu_reference_keeps_the_negative_tail():
    """0.5 x erfc(-x / sqrt 2) against the closed asymptotic form -phi(x) (1 - 1 / x^2 + 3 / x^4) at x = -12: no cancellation"""
    x = torch.tensor([-12.0], dtype=torch.float64)
    want = -torch.exp(-x * x / 2) / np.sqrt(2 * np.pi) * (1 - 1 / x ** 2 + 3 / x ** 4)
    assert abs(float(NE.act64(x, "gelu") / want) - 1.0) < 1e-3
    assert float(NE.act64(torch.tensor([-20.0]), "gelu")) < 0.0                     # 1 + erf would give exactly 0


# ---------------------------------------------------------------------------------------------------------------------- emulations pass
@pytest.mark.parametrize("name,act", [("silu_f", "silu"), ("silu_fast", "silu"), ("gelu_f", "gelu")])
def test_fp32_emulation_of_the_shipped_formula_passes(name, act):
    x = NE.sweep()["x"]
    got = NE.as_stored(getattr(NE, "emu_" + name)(x.numpy()))
    ref, bound = NE.sweep_ref(act)
    ratio = U.check_elem(got, ref, bound, "emulated " + name, NE.locate_point)
    assert ratio < 0.75, ratio              # 0.500 / 0.500 / 0.557 (at x = -3.296) when this was written: half an ulp16 of rounding and little else


def test_geglu_emulation_passes():
    x = NE.sweep()["x"]
    u = np.array([NE.GEGLU_U[q % 3] for q in range(NE.CH)], np.float32)[None, :]
    got = NE.as_stored((u * NE.emu_gelu_f(x.numpy())).astype(np.float32))
    ref, bound = NE.geglu_sweep_ref()
    assert U.check_elem(got, ref, bound, "emulated GEGLU", NE.locate_point) < 0.75


# ---------------------------------------------------------------------------------------------------------------------- planted mistakes fail
@pytest.mark.parametrize("name,floor", [("tanh_gelu", 8000), ("quick_gelu", 60000), ("silu_for_gelu", 90000)])
def test_planted_activation_mistake_is_rejected(name, floor):
    """measured when this was written: 9 800 / 73 789 / 101 399 of the 253 952 points (a quarter of that in distinct halves), at 0.00095 <= |x| <= 16.4;
    1 232 / 4 994 / 11 836 of them beyond |x| = 4"""
    x = NE.sweep()["x"]
    wrong = dict(tanh_gelu=NE.planted_tanh_gelu, quick_gelu=NE.planted_quick_gelu, silu_for_gelu=NE.emu_silu_f)[name](x.numpy())
    got = NE.as_stored(wrong)
    ref, bound = NE.sweep_ref("gelu")
    with pytest.raises(AssertionError):
        U.check_elem(got, ref, bound, name, NE.locate_point)
    bad = (got.double() - ref).abs() > U.ulp16(ref) + bound
    assert int(bad.sum()) >= floor, int(bad.sum())
    assert float(x[bad].abs().max()) > 4.0, "some of the rejecting points lie beyond what N(0, 1) data reaches"
    gauss = x.abs() <= 4.0
    assert int((bad & ~gauss).sum()) > 0


def test_gn_silu_case_reaches_large_arguments_and_the_subnormal_zone():
    c = NE.gn_silu_case()
    assert float(c["pre"].max()) > 1000.0 and float(c["pre"].min()) < -400.0
    sub = (c["ref"].abs() < 2.0 ** -14) & (c["ref"].abs() > 2.0 ** -25)
    assert int(sub.sum()) > 50, int(sub.sum())                                     # results that are fp16 subnormals
    assert bool(torch.isfinite(c["ref"].half()).all())


# ---------------------------------------------------------------------------------------------------------------------- norms: discrimination
def _gn_onepass_fp32(x, n, HW, gamma, beta, eps, clamp=True):
    """fp32 emulation of the library's one-pass GroupNorm: sums of x and x^2 per group, var = max(q / n - m^2, 0), affine in fp32, fp16 store"""
    C = x.shape[1]
    gs = C // NE.GROUPS
    xg = x.float().reshape(n, HW, NE.GROUPS, gs)
    s, q = xg.sum((1, 3), dtype=torch.float32), (xg * xg).sum((1, 3), dtype=torch.float32)
    inv = np.float32(1.0) / np.float32(gs * HW)
    mean = s * inv
    var = q * inv - mean * mean
    if clamp:
        var = var.clamp_min(0.0)
    r = torch.rsqrt(var + np.float32(eps))
    per_ch = lambda t: t[:, None, :, None].expand(n, HW, NE.GROUPS, gs).reshape(n * HW, C)
    sc = gamma.float()[None, :] * per_ch(r)
    sh = beta.half().float()[None, :] - per_ch(mean) * sc
    return (x.float() * sc + sh).half()


@pytest.mark.parametrize("eps", NE.EPS_VALUES)
@pytest.mark.parametrize("name,c0,c1,HW", NE.GN_SHAPES + [("rows%d" % hw, 64, 0, hw) for hw, _ in NE.GN_ROWS[1:]])
def test_group_norm_eps_cases_tell_one_eps_from_another(name, c0, c1, HW, eps):
    x, gamma, beta, ref, bound = NE.gn_case("eps", c0, c1, HW, eps, 0)
    for other in (NE.other_eps(eps), 1e-12):
        d = NE.discrimination(ref, bound, NE.gn_case("eps", c0, c1, HW, other, 0)[3])
        assert d >= MIN_DISCRIMINATION, (name, eps, other, d)
    got = _gn_onepass_fp32(x, 2, HW, gamma, beta, eps)
    assert U.check_elem(got, ref, bound, "one-pass emulation %s eps %g" % (name, eps)) < 1.0
    with pytest.raises(AssertionError):
        U.check_elem(_gn_onepass_fp32(x, 2, HW, gamma, beta, NE.other_eps(eps)), ref, bound, "emulation with the other eps")


@pytest.mark.parametrize("kind", ["const", "zero"])
def test_group_norm_constant_groups_need_the_clamp(kind):
    """the emulation passes on constant and zero groups with the clamp; without it some constant group has a negative fp32 variance beyond eps"""
    x, gamma, beta, ref, bound = NE.gn_case(kind, 64, 0, 384, 1e-6, 0)
    got = _gn_onepass_fp32(x, 2, 384, gamma, beta, 1e-6)
    assert U.check_elem(got, ref, bound, "one-pass emulation " + kind) < 1.0
    if kind == "zero":
        assert torch.equal(got, beta.half()[None, :].expand_as(got))
    else:
        assert not bool(torch.isfinite(_gn_onepass_fp32(x, 2, 384, gamma, beta, 1e-6, clamp=False)).all())


@pytest.mark.parametrize("eps", NE.EPS_VALUES)
@pytest.mark.parametrize("C,rows", NE.LN_SHAPES)
def test_layer_norm_eps_cases_tell_one_eps_from_another(C, rows, eps):
    _, _, _, ref, bound = NE.ln_case("eps", rows, C, eps)
    for other in (NE.other_eps(eps), 1e-12):
        d = NE.discrimination(ref, bound, NE.ln_case("eps", rows, C, other)[3])
        assert d >= MIN_DISCRIMINATION, (C, rows, eps, other, d)


@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("C", [8, 72, 512, 520])
def test_l2norm_rows_depend_on_the_hard_coded_eps(C, half):
    x = NE.l2norm_rows(C, 2800 + C, half)
    ref, bound = HC.l2norm_ref_bound(x)
    assert torch.equal(ref, NE.l2norm_ref(x, 1e-6))
    live = [0, 1, 2, 3]
    for other in (1e-5, 1e-12):
        d = NE.discrimination(ref[live], bound[live], NE.l2norm_ref(x, other)[live], out_f32=not half)
        assert d >= MIN_DISCRIMINATION, (C, half, other, d)
    ss = (x.double() ** 2).sum(-1)
    assert 0.4e-6 < float(ss[1]) < 0.6e-6 and 0.9e-6 < float(ss[0]) < 1.1e-6 and float(ss[3]) == C * 2.0 ** -28 and float(ss[4]) == 0.0


@pytest.mark.parametrize("eps", NE.EPS_VALUES)
def test_linear_behind_a_norm_tells_one_eps_from_another(eps):
    *_, ref, bound = NE.ln_linear_case("eps", eps)
    *_, gref, gbound = NE.gn_linear_case("eps", eps)
    for other in (NE.other_eps(eps), 1e-12):
        d = NE.discrimination(ref, bound, NE.ln_linear_case("eps", other)[5])
        assert d >= MIN_DISCRIMINATION, ("ln", eps, other, d)
        d = NE.discrimination(gref, gbound, NE.gn_linear_case("eps", other)[4])
        assert d >= MIN_DISCRIMINATION, ("gn", eps, other, d)


def test_fused_blocks_tell_one_eps_from_another():
    """judged by rel-L2 < XF_TOL like the existing tests of these kernels: the reference with another ln_eps must be several tolerances away"""
    for case in (NE.xattn_case, NE.ff_case):
        ref = case(1e-6)["ref"]
        for other in (1e-5, 1e-12):
            assert U.rel_l2(case(other)["ref"], ref) > 5 * NE.XF_TOL, (case.__name__, other, U.rel_l2(case(other)["ref"], ref))


# ---------------------------------------------------------------------------------------------------------------------- the VAE's eps s^2
def _vae_k_conditions(k):
    vcfg, sd0, z = NE.vae_tiny()
    sd = NE.vae_scaled_state_dict(sd0, k)
    ref, rms = NE.vae_decode_with_eps(sd, vcfg, z)
    wrong, _ = NE.vae_decode_with_eps(sd, vcfg, z, 4.0 ** NE.VAE_SHIFT)           # an unscaled eps against a stream stored x 2^-4
    return U.psnr(wrong, ref), 2.0 ** -NE.VAE_SHIFT * min(rms)                   # rms is of the stream as scaled by F already


def test_vae_scale_exponent_is_the_largest_that_meets_both_conditions():
    """measured when this was written: k = 6 -> 28.6 dB with eps x 256 and a shifted stream rms of 1.01e-3 (> 2^-10 = 0.98e-3); k = 7 -> 0.50e-3:
    out of the range condition; k = 3 would still pass with the wrong eps (59.5 dB)"""
    assert len(NE.vae_decode_with_eps(*[NE.vae_tiny()[i] for i in (1, 0, 2)])[1]) >= 10       # the hook sees the stream-reading norms
    psnr_wrong, shifted_rms = _vae_k_conditions(NE.VAE_K)
    assert psnr_wrong < NE.VAE_PSNR_DB, psnr_wrong
    assert shifted_rms > 2.0 ** -10, shifted_rms
    _, shifted_rms_next = _vae_k_conditions(NE.VAE_K + 1)
    assert shifted_rms_next <= 2.0 ** -10, shifted_rms_next
