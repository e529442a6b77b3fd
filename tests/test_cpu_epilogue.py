"""Self-test of the epilogue / batched-GEMM bounds (tests/util.py conv_ref_bound, gemm_batched_ref_bound) on the CPU.

tests/epilogue_cases.py emulates the kernels' arithmetic in torch fp32 -- fp16 operands, fp32 accumulation, roundings at exactly the
points the bounds' derivation lists.  For every case tests/test_gpu_epilogue.py judges on the GPU:
  * the faithful emulation passes check_elem with the derived bound: the reference alone stays inside its bound;
  * every mutant -- one mistake an epilogue could make with the fields only the VAE, the time embedding and the batched callers use --
    fails it: the inputs are lively enough for the per-element check to see the mistake."""
import pytest
import torch

from tests import epilogue_cases as E
from tests import util as U


def _judge_conv(c, what, **kw):
    return U.check_elem(E.emulate_conv(c, **kw).float(), c.ref, c.bound, what)


@pytest.mark.parametrize("out_scale,mask", E.RANGE_GUARD)
def test_range_guard_emulation_is_inside_the_bound(out_scale, mask):
    assert _judge_conv(E.range_guard_case(out_scale, mask), "range guard") <= 1.0


@pytest.mark.parametrize("act", ["silu", "gelu", "relu"])
def test_deep_k_emulation_is_inside_the_bound(act):
    c = E.deep_k_case(act)
    assert _judge_conv(c, "deep K " + act) <= 1.0
    if act == "silu":
        assert _judge_conv(c, "deep K rowadd_idx", rowadd_from_table=True) <= 1.0


def test_gelu_reference_is_the_exact_erf_form():
    """conv_ref_bound's GELU is F.gelu in float64 (exact erf), not the tanh form: the two differ by up to 5e-4, far above the bound"""
    x = torch.linspace(-4, 4, 4001, dtype=torch.float64)
    exact = 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))
    assert float((U._act64(x, "gelu") - exact).abs().max()) < 1e-15


@pytest.mark.parametrize("mutant", [m for m in E.CONV_MUTANTS if m not in ("bias_mul_on_rowadd", "wrong_rowadd_row")])
@pytest.mark.parametrize("out_scale,mask", E.RANGE_GUARD)
def test_range_guard_mutants_fail(out_scale, mask, mutant):
    with pytest.raises(AssertionError, match="outside ulp16|non-finite"):
        _judge_conv(E.range_guard_case(out_scale, mask), mutant, mutant=mutant)


@pytest.mark.parametrize("mutant", E.CONV_MUTANTS)
def test_deep_k_mutants_fail(mutant):
    """the split-K / rowadd_idx problem carries every field: every mutant is visible on it, the time-embedding ones only here"""
    with pytest.raises(AssertionError, match="outside ulp16|non-finite"):
        _judge_conv(E.deep_k_case("silu"), mutant, mutant=mutant, rowadd_from_table=True)


def test_an_activation_mix_up_fails():
    """SiLU, GELU and ReLU differ by far more than the bound on these inputs: a kernel that runs the wrong one cannot pass"""
    g, r = E.deep_k_case("gelu"), E.deep_k_case("relu")
    for c, other in ((g, "relu"), (g, "silu"), (r, "gelu")):
        saved, c.act = c.act, other
        try:
            with pytest.raises(AssertionError, match="outside ulp16"):
                _judge_conv(c, "%s run as %s" % (saved, other))
        finally:
            c.act = saved


def _judge_batched(c, what, mutant=None):
    return U.check_elem(E.emulate_batched(c, mutant).float(), c.ref, c.bound, what, out_f32=c.out_f32)


@pytest.mark.parametrize("name", E.BATCH_CASES)
def test_batched_emulation_is_inside_the_bound(name):
    assert _judge_batched(E.batch_case(name), name) <= 1.0


@pytest.mark.parametrize("name,mutant", [("vae_vt", "pixel_bias_by_channel"), ("batched_residual", "bs_res_for_bs_out"), ("vit_patch_embed", "bs_res_for_bs_out")]
                         + [(n, "batch_reads_element0") for n in E.BATCH_CASES])
def test_batched_mutants_fail(name, mutant):
    with pytest.raises(AssertionError, match="outside ulp16|non-finite"):
        _judge_batched(E.batch_case(name), "%s %s" % (name, mutant), mutant)


def test_fp32_output_is_judged_at_fp32_resolution():
    """check_elem(out_f32=True) grants U32 |ref| for the stored value: an error of one fp16 ulp, which the fp16 check lets pass, fails it"""
    c = E.batch_case("vae_scores")
    got = E.emulate_batched(c).double()
    off = got + U.ulp16(c.ref) * 0.9
    U.check_elem(off, c.ref, c.bound, "fp16 resolution")
    with pytest.raises(AssertionError, match="outside ulp16"):
        U.check_elem(off, c.ref, c.bound, "fp32 resolution", out_f32=True)


def test_guarded_batch_layout():
    """guarded_batch: the rows between two elements are poison, a write there is found, the batch stride is a multiple of 8 elements"""
    ts = [E.rand((5, 12), 900 + b).half() for b in range(3)]
    g = U.guarded_batch(ts, ld=20, gap_rows=1, device="cpu")
    assert g.bs % 8 == 0 and g.bs > 5 * 20
    assert torch.equal(g.cpu(), torch.stack(ts))
    U.assert_untouched(g, "fresh")
    assert int((~g.poison_mask()).sum()) == 3 * 5 * 12
    g.buf[g.pre * 20 + 5 * 20 + 3] = 1.0            # first gap row behind element 0
    with pytest.raises(AssertionError, match="poison elements were overwritten"):
        U.assert_untouched(g, "gap write")
