"""Self-attention guidance on the host, no GPU: the reference's own properties (tests/sag_ref.py), the conditioning of the inputs the GPU
tests use (the peaked checkpoint gives a mask that is neither empty nor full and mostly outside the fp16 band), the plain-loop identity,
the host plan's refusals (ladi_tryon_plan_forms_sag, the plan_evals that TryOn::run calls) and the pipeline's argument checks."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd.pipeline import sag_check
from ladi_vton_amd import schedulers as SCH
from oracle import configs as C
from oracle import pipeline as P
from tests import ref_tryon as RT
from tests import sag_ref as S
from tests import util as U

# the forward inputs and loop inputs of tests/test_gpu_sag.py
FWD_SIZES = [(64, 48), (52, 38)]
T0 = 481.0
BAND_SHARE = 0.15
SAG_WITH_FEATURE_CACHE, SAG_WITH_PAG, SAG_TOME_MID, SAG_SCHEDULER, SAG_SMALL = -14, -15, -16, -17, -18


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


@pytest.fixture(scope="module")
def unet():
    cfg = C.UNET_TINY
    return cfg, S.peaked(C.synth_state_dict(C.unet_shapes(cfg), "unet."))


def fwd_inputs(cfg, hw, n=2):
    """tests/tiny_tryon.py unet_inputs' draws (n different samples)"""
    g = torch.Generator().manual_seed(11 + hw[0])
    x = torch.randn((n, 31) + hw, generator=g).half().float()
    ehs = torch.randn((n, 8, cfg["cross_attention_dim"]), generator=g).half().float()
    return x, ehs


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def test_taps_sum_to_one():
    t = S.taps()
    assert t.shape == (9,) and abs(float(t.sum()) - 1.0) <= 1e-15
    assert torch.equal(t, t.flip(0)) and float(t[4]) == float(t.max())
    assert abs(float(t[3] / t[4]) - math.exp(-0.5)) <= 1e-15


@pytest.mark.parametrize("hw", [(5, 5), (6, 5), (13, 9), (64, 48)])
def test_blur_of_a_constant_is_the_constant(hw):
    x = torch.full((2, 4) + hw, 0.37, dtype=torch.float64)
    assert float((S.blur9(x) - 0.37).abs().max()) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("hw", [(5, 5), (6, 5), (13, 9), (64, 48)])
def test_blur_is_the_dense_convolution_of_the_reflect_padded_input(hw):
    """the separable passes against one dense 9 x 9 F.conv2d with the outer-product kernel, in float64: rounding of another summation order"""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn((2, 4) + hw, generator=g, dtype=torch.float64)
    t = S.taps()
    k2 = torch.outer(t, t)
    w = torch.zeros((4, 4, 9, 9), dtype=torch.float64)
    for c in range(4):
        w[c, c] = k2
    dense = F.conv2d(F.pad(x, (4, 4, 4, 4), mode="reflect"), w)
    assert S.blur9(x).shape == x.shape
    assert float((S.blur9(x) - dense).abs().max()) <= 64 * 2.0 ** -53 * float(x.abs().max())
    # reflect, not replicate: the pixel left of column 0 is column 1
    assert torch.equal(F.pad(x, (4, 4, 4, 4), mode="reflect")[..., 4:-4, 3], x[..., 1])


@pytest.mark.parametrize("a", [0.9991, 0.5, 0.0047])
def test_degrade_with_an_empty_mask_is_the_x0_round_trip(a):
    """m = 0: xd = sqrt(a) ((x - sqrt(1 - a) b) / sqrt(a)) + sqrt(1 - a) b = x up to the rounding of the round trip: each of the four
    operations rounds once, relative to |x| + sqrt(1 - a) |b|"""
    g = torch.Generator().manual_seed(3)
    x, b = torch.randn((2, 4, 13, 9), generator=g), torch.randn((2, 4, 13, 9), generator=g)
    xd = S.degrade(x, b, torch.zeros((2, 2, 2), dtype=torch.uint8), a)
    bound = 4 * 2.0 ** -24 * (x.abs() + math.sqrt(1 - a) * b.abs()) * 2
    assert bool(((xd - x).abs() <= bound).all())
    # and with a full mask it is another tensor
    assert float((S.degrade(x, b, torch.ones((2, 2, 2), dtype=torch.uint8), a) - x).abs().max()) > 1e-3


def test_upsampled_mask_follows_the_nearest_index_rule():
    m = torch.arange(6).reshape(1, 2, 3) % 2
    up = S.upsampled(m, 13, 9)[0, 0]
    from tests import ref_unet as RU
    for y in range(13):
        for x in range(9):
            assert up[y, x] == m[0, RU.nearest_src(y, 2, 13), RU.nearest_src(x, 3, 9)]


def test_combine_forms():
    g = torch.Generator().manual_seed(5)
    eu, ec, ed = (torch.randn((2, 4, 8, 6), generator=g, dtype=torch.float64) for _ in range(3))
    assert torch.equal(S.combine(eu, ec, ed, 7.5, 0.0), eu + 7.5 * (ec - eu))
    assert torch.equal(S.combine(None, ec, ed, 7.5, 0.0), ec)
    assert torch.allclose(S.combine(eu, ec, ed, 7.5, 0.75), eu + 7.5 * (ec - eu) + 0.75 * (eu - ed), rtol=0, atol=1e-14)
    assert torch.allclose(S.combine(None, ec, ed, 1.0, 0.75), ec + 0.75 * (ec - ed), rtol=0, atol=1e-14)
    r = S.combine(eu, ec, ed, 7.5, 0.75, phi=1.0)
    assert abs(float(r[0].std() / ec[0].std()) - 1.0) <= 1e-12          # phi = 1: the whole sum takes the cond prediction's std


# ------------------------------------------------------------------------------------------------------------------ input conditioning
@pytest.mark.parametrize("hw", FWD_SIZES)
def test_forward_inputs_are_conditioned(unet, hw):
    """for the forward inputs of the GPU tests: the reference mask has between 10 % and 90 % ones and at most 15 % of the tokens lie inside
    the band (twice the float32-against-fp16 difference of the reference) in which the library's mask is not pinned"""
    cfg, sd = unet
    x, ehs = fwd_inputs(cfg, hw)
    s, band = S.band_of(sd, cfg, x, T0, ehs)
    ones = float(S.mask_of(s).float().mean())
    share = float(((s - 1.0).abs() <= band).float().mean())
    print("SAG conditioning %dx%d: T = %d, ones %.2f, band %.4g, share inside %.3f" % (hw + (s.shape[1], ones, band, share)))
    assert s.shape == (2, math.prod(S.map_size(*hw)))
    assert 0.10 <= ones <= 0.90 and share <= BAND_SHARE, (ones, band, share)
    assert float((s.sum(dim=1) - s.shape[1]).abs().max()) <= 1e-3            # every row of P sums to 1


def loop_inputs(B, H, W, D):
    inp = P.synthetic_inputs(B, H, W, L=8, D=D)
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp


@pytest.fixture(scope="module")
def tiny_sd(unet):
    vcfg = C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    return dict(ucfg=unet[0], unet=unet[1], vcfg=vcfg, vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
                emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))


@pytest.mark.parametrize("H,W,steps", [(256, 192, 3), (512, 384, 6)])
def test_loop_masks_are_conditioned(tiny_sd, H, W, steps):
    """the loops of the GPU tests (B = 2, DDIM, CFG, sag_scale 0.75; latents 32 x 24 with 3 steps and 64 x 48 with 6): every evaluation's
    own mask has between 10 % and 90 % ones"""
    inp = loop_inputs(2, H, W, tiny_sd["ucfg"]["cross_attention_dim"])
    info = {}
    S.tryon_sag_reference(tiny_sd["unet"], tiny_sd["ucfg"], tiny_sd["vae"], tiny_sd["vcfg"], tiny_sd["emasc"], inp, steps, "ddim", sag_scale=0.75,
                          info=info)
    assert len(info["masks"]) == steps
    for i, m in enumerate(info["masks"]):
        ones = float(m.float().mean())
        print("SAG loop %dx%d evaluation %d: ones %.2f" % (H, W, i, ones))
        assert m.shape == (2,) + S.map_size(H // 8, W // 8) and 0.10 <= ones <= 0.90, (i, ones)


# ------------------------------------------------------------------------------------------------------------------ plain-loop identity
@pytest.mark.parametrize("kw", [dict(scheduler="ddim"), dict(scheduler="pndm", phi=0.7), dict(scheduler="ddim", table=[7.5, 1.0, 7.5])],
                         ids=["ddim", "pndm_rescale", "cutoff"])
def test_scale_zero_is_the_plain_reference_bit_for_bit(tiny_sd, kw):
    kw = dict(kw)
    sched = kw.pop("scheduler")
    steps = 3 if sched == "ddim" else 2
    inp = loop_inputs(1, 64, 48, tiny_sd["ucfg"]["cross_attention_dim"])
    a = (tiny_sd["unet"], tiny_sd["ucfg"], tiny_sd["vae"], tiny_sd["vcfg"], tiny_sd["emasc"], inp, steps, sched)
    img_r, lat_r = RT.tryon_reference(*a, **kw)
    img_s, lat_s = S.tryon_sag_reference(*a, sag_scale=0.0, **kw)
    assert torch.equal(lat_r, lat_s) and torch.equal(img_r, img_s)


# ------------------------------------------------------------------------------------------------------------------ host plan
def plan(lib, evals, sag, sched=SCH.DDIM, hw=(64, 48), mid_merges=0, guidance=7.5, table=None, phi=0.0, pag=None, flags=None):
    def arr(ctype, v):
        return ((ctype * len(v))(*v), len(v)) if v is not None else (None, 0)
    out = (ctypes.c_ubyte * max(evals, 1))()
    rc = lib.ladi_tryon_plan_forms_sag(evals, 0, evals, guidance, *arr(ctypes.c_float, table), phi, *arr(ctypes.c_float, pag),
                                       *arr(ctypes.c_ubyte, flags), sag, sched, hw[0], hw[1], mid_merges, out)
    return list(out[:evals]) if rc == evals else (rc, _lib.last_error())


def plain(lib, evals, **kw):
    def arr(ctype, v):
        return ((ctype * len(v))(*v), len(v)) if v is not None else (None, 0)
    out = (ctypes.c_ubyte * evals)()
    rc = lib.ladi_tryon_plan_forms(evals, 0, evals, kw.get("guidance", 7.5), *arr(ctypes.c_float, kw.get("table")), kw.get("phi", 0.0), None, 0,
                                   None, 0, out)
    assert rc == evals
    return list(out)


def test_plan_forms_are_the_plain_runs(lib):
    for kw in (dict(), dict(guidance=1.0), dict(table=[7.5, 7.5, 1.0, 1.0, 7.5]), dict(phi=0.7), dict(table=[1.0] * 5)):
        assert plan(lib, 5, 0.75, **kw) == plain(lib, 5, **kw) == plan(lib, 5, 0.0, **kw)
    assert plan(lib, 6, 0.75, sched=SCH.PNDM) == [0] * 6
    for sched in (SCH.DDIM, SCH.PNDM, SCH.DPMPP, SCH.LCM, SCH.TCD):
        assert plan(lib, 4, 0.75, sched=sched) == [0] * 4
    assert plan(lib, 4, 0.75, hw=(5, 5)) == [0] * 4


def test_plan_refusals(lib):
    rc, msg = plan(lib, 4, 0.75, flags=[1, 0, 1, 0])
    assert rc == SAG_WITH_FEATURE_CACHE and "feature-cache plan" in msg and "mid block" in msg
    rc, msg = plan(lib, 4, 0.75, flags=[1, 1, 1, 1])
    assert rc == SAG_WITH_FEATURE_CACHE
    rc, msg = plan(lib, 4, 0.75, pag=[0.0, 0.0, 1e-3, 0.0])
    assert rc == SAG_WITH_PAG and "PAG" in msg
    assert plan(lib, 4, 0.75, pag=[0.0] * 4) == [0] * 4                       # a table of zeros is no PAG
    rc, msg = plan(lib, 4, 0.75, mid_merges=1)
    assert rc == SAG_TOME_MID and "token merging" in msg
    for sched, name in ((SCH.EULER, "Euler"), (SCH.EULER_ANCESTRAL, "Euler-ancestral"), (SCH.LMS, "LMS")):
        rc, msg = plan(lib, 4, 0.75, sched=sched)
        assert rc == SAG_SCHEDULER and name in msg, (sched, rc, msg)
        assert plan(lib, 4, 0.0, sched=sched) == [0] * 4                        # off: nothing is refused
    for hw in ((4, 48), (64, 4), (1, 1)):
        rc, msg = plan(lib, 4, 0.75, hw=hw)
        assert rc == SAG_SMALL and "5 x 5" in msg and "%d x %d" % hw in msg
    assert plan(lib, 4, 0.0, flags=[1, 0, 1, 0], hw=(1, 1), mid_merges=1) == [0, 2, 0, 2]
    assert plan(lib, 4, -1.0)[0] == -1 and plan(lib, 4, float("nan"))[0] == -1


def test_pipeline_argument_checks():
    ok = dict(scheduler=SCH.DDIMScheduler(), latent_size=(64, 48))
    assert sag_check(0.75, **ok) == 0.75 and sag_check(0, **ok) == 0.0
    assert sag_check(0.0, scheduler=SCH.EulerDiscreteScheduler(), latent_size=(1, 1), feature_cache=2) == 0.0
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="sag_scale"):
            sag_check(bad, **ok)
    with pytest.raises(ValueError, match="feature_cache"):
        sag_check(0.75, feature_cache=2, **ok)
    with pytest.raises(ValueError, match="pag_scale"):
        sag_check(0.75, pag_table=[0.0, 3.0], **ok)
    assert sag_check(0.75, pag_table=[0.0, 0.0], **ok) == 0.75
    for cls in (SCH.EulerDiscreteScheduler, SCH.EulerAncestralDiscreteScheduler, SCH.LMSDiscreteScheduler):
        with pytest.raises(ValueError, match=cls.__name__):
            sag_check(0.75, scheduler=cls(), latent_size=(64, 48))
    with pytest.raises(ValueError, match="5 x 5"):
        sag_check(0.75, scheduler=SCH.DDIMScheduler(), latent_size=(4, 6))
    from ladi_vton_amd import tome
    assert sag_check(0.75, tome_cfg=tome.config(ratio=0.5, max_downsample=2), **ok) == 0.75      # the outer levels only: the mid block never merges
