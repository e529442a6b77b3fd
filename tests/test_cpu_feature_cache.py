"""Deep-feature cache (DeepCache on the full-resolution level), host side: the reference's self-checks, the plan and its promotion rule,
every ValueError of the Python interface, the exports, and the reference loop's counts.  The device side is tests/test_gpu_feature_cache.py."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P
from tests import feature_cache_ref as R
from tests import ref_tryon as RT
from tests import ref_unet as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    return dict(ucfg=ucfg, vcfg=vcfg, unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
                emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))


def _unet_case(tiny, hw=(16, 8), n=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 31) + hw, generator=g)
    ehs = torch.randn((n, 8, tiny["ucfg"]["cross_attention_dim"]), generator=g)
    return x, ehs


# ------------------------------------------------------------------------------------------------------------------ reference self-checks
def test_reference_whole_forward_is_the_oracle_forward(tiny):
    x, ehs = _unet_case(tiny)
    want = M.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs)
    assert torch.equal(RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs), want)
    for k in (0, 1, 2):
        out, cap = RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs, cache=("capture", k))
        assert torch.equal(out, want)
        assert cap.shape == (2, tiny["ucfg"]["block_out_channels"][1 if k == 2 else 0], 16, 8)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_shallow_at_the_captured_input_is_the_whole_forward(tiny, k):
    """the same layers on the same tensors: exactly equal; at another input and timestep it is another function (the comparison sees it)"""
    x, ehs = _unet_case(tiny)
    want, cap = RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs, cache=("capture", k))
    assert torch.equal(RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs, cache=("shallow", k, cap)), want)
    x1, _ = _unet_case(tiny, seed=4)
    other = RU.unet_forward(tiny["unet"], tiny["ucfg"], x1, 461, ehs, cache=("shallow", k, cap))
    whole1 = M.unet_forward(tiny["unet"], tiny["ucfg"], x1, 461, ehs)
    assert not torch.equal(other, whole1) and not torch.equal(other, want) and torch.isfinite(other).all()


def test_reference_cache_point_differs_per_branch_and_runs_odd_sizes(tiny):
    x, ehs = _unet_case(tiny, hw=(13, 10))
    caps = [RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs, cache=("capture", k))[1] for k in (0, 1, 2)]
    assert all(c.shape[-2:] == (13, 10) for c in caps)
    assert not torch.equal(caps[0], caps[1]) and not torch.equal(caps[1], caps[2])
    want = RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs)
    for k in (0, 1, 2):
        assert torch.equal(RU.unet_forward(tiny["unet"], tiny["ucfg"], x, 481, ehs, cache=("shallow", k, caps[k])), want)


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_feature_cache_plan_interval_forms():
    import ladi_vton_amd as L
    assert L.feature_cache_plan(7, 1) == [True] * 7
    assert L.feature_cache_plan(7, 2) == [True, False, True, False, True, False, True]
    assert L.feature_cache_plan(7, 3) == [True, False, False, True, False, False, True]
    assert L.feature_cache_plan(3, 50) == [True, False, False]
    assert L.feature_cache_plan(0, 2) == []
    # a sequence: truthy / falsy entries, flag 0 forced
    assert L.feature_cache_plan(4, [0, 0, 1, ""]) == [True, False, True, False]
    assert L.feature_cache_plan(3, (False, True, False)) == [True, True, False]
    for n in (1, 6, 7):
        for N in (1, 2, 3, 5):
            assert L.feature_cache_plan(n, N) == R.plan(n, N)


def test_feature_cache_plan_promotion_under_a_guidance_interval():
    """CFG on the middle of the run: evaluations 0-1 and 6-7 run cond-only.  A shallow CFG evaluation whose last whole evaluation was
    cond-only is promoted; shallow cond-only evaluations never are; after the promoted (whole, CFG) evaluation the plan goes on as given"""
    import ladi_vton_amd as L
    table = L.guidance_interval(8, 7.5, 0.25, 0.75)
    co = [not g > 1.0 for g in table]
    assert co == [True, True, False, False, False, False, True, True]
    #            i:  0     1      2     3      4     5      6     7
    # interval 3:    W     s      s->W  W      s     s      W     s         (2: last whole was 0, cond-only -> promoted)
    assert L.feature_cache_plan(8, 3, co) == [True, False, True, True, False, False, True, False]
    # interval 4:    W     s      s->W  s      W     s      s     s         (3 follows the promoted whole CFG evaluation: stays shallow;
    #                                                                        6, 7 are cond-only: never promoted)
    assert L.feature_cache_plan(8, 4, co) == [True, False, True, False, True, False, False, False]
    # a whole cond-only evaluation late in the run, then CFG again
    co2 = [False, False, True, False, False]
    assert L.feature_cache_plan(5, [1, 0, 1, 0, 0], co2) == [True, False, True, True, False]
    # without cond-only evaluations nothing is promoted, and a run that is cond-only throughout promotes nothing either
    assert L.feature_cache_plan(8, 3, [False] * 8) == L.feature_cache_plan(8, 3)
    assert L.feature_cache_plan(8, 3, [True] * 8) == L.feature_cache_plan(8, 3)
    for N in (2, 3, 4, 5):
        assert L.feature_cache_plan(8, N, co) == R.plan(8, N, co)


def test_feature_cache_value_errors():
    import ladi_vton_amd as L
    from ladi_vton_amd.pipeline import feature_cache_spec
    for bad in (0, -2, 2.5, True, "x"):
        with pytest.raises(ValueError, match="interval|sequence|entries"):
            L.feature_cache_plan(6, bad)
    with pytest.raises(ValueError, match="3 entries but the scheduler runs 6"):
        L.feature_cache_plan(6, [1, 0, 1])
    with pytest.raises(ValueError, match="cond_only"):
        L.feature_cache_plan(6, 2, [True])
    for bad in (-1, 3, 1.0, True, None):
        with pytest.raises(ValueError, match="branch"):
            feature_cache_spec({"interval": 2, "branch": bad}, 6)
    with pytest.raises(ValueError, match="keys"):
        feature_cache_spec({"interval": 2, "every": 3}, 6)
    with pytest.raises(ValueError, match="keys"):
        feature_cache_spec({"branch": 1}, 6)
    with pytest.raises(ValueError, match="interval"):
        feature_cache_spec({"interval": 0}, 6)
    # what it returns: off, the plain run for N = 1 / all true (capture is not even switched on), else the flags and the branch
    assert feature_cache_spec(None, 6) == (None, 0)
    assert feature_cache_spec(1, 6) == (None, 0) and feature_cache_spec([1] * 6, lambda: 6) == (None, 0)
    assert feature_cache_spec(3, 6) == ([True, False, False, True, False, False], 0)
    assert feature_cache_spec({"interval": 2, "branch": 2}, 4) == ([True, False, True, False], 2)
    assert feature_cache_spec({"interval": [1, 0, 0]}, 3) == ([True, False, False], 0)


def test_feature_cache_needs_the_native_unet():
    """the pipeline refuses `feature_cache` with another UNet before any work (no GPU is touched)"""
    import ladi_vton_amd as L
    pipe = L.StableDiffusionTryOnePipeline(vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=[1, 2, 3, 4])), text_encoder=None,
                                           tokenizer=None, unet=SimpleNamespace(config=SimpleNamespace(sample_size=8)), scheduler=L.DDIMScheduler())
    kw = dict(image=torch.zeros(1, 3, 64, 64), mask_image=torch.zeros(1, 1, 64, 64), pose_map=None, warped_cloth=None,
              prompt_embeds=torch.zeros(1, 2, 4), height=64, width=64, num_inference_steps=6)
    with pytest.raises(ValueError, match="native UNet"):
        pipe(feature_cache=2, **kw)
    with pytest.raises(ValueError, match="native UNet"):
        pipe(feature_cache=1, **kw)
    with pytest.raises(ValueError, match="7 entries but the scheduler runs 6"):
        pipe(feature_cache=[1] * 7, **kw)
    with pytest.raises(ValueError, match="branch"):
        pipe(feature_cache={"interval": 2, "branch": 5}, **kw)
    assert pipe.shallow_evals is None


# ------------------------------------------------------------------------------------------------------------------ exports
NEW_SYMBOLS = ("ladi_tryon_set_feature_cache", "ladi_tryon_shallow_evals", "ladi_unet_forward_cached", "ladi_unet_forward_cached_rows",
               "ladi_unet_time_forward_cached")


def test_new_symbols_are_declared_and_typed():
    from ladi_vton_amd import _lib
    header = open(os.path.join(ROOT, "include", "ladi_native.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    # the argument counts of the ctypes mirrors are the header's
    for name in NEW_SYMBOLS:
        args = re.search(r"\bint %s\(([^;]*)\);" % name, header, re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the existing input struct keeps its layout: the feature is set through its own call
    assert "feature" not in re.search(r"typedef struct \{[^}]*\} ladi_tryon_inputs;", header, re.S).group(0)


# ------------------------------------------------------------------------------------------------------------------ the reference loop
def _loop_inputs(tiny, B=1, H=64, W=64):
    return P.synthetic_inputs(B, H, W, L=8, D=tiny["ucfg"]["cross_attention_dim"])


def _loop(tiny, inp, interval, branch=0, steps=4, sched="ddim", table=None, counts=None):
    return RT.tryon_reference(tiny["unet"], tiny["ucfg"], tiny["vae"], tiny["vcfg"], tiny["emasc"], inp, steps, sched, table=table,
                              feature_cache=(interval, branch), info=counts)


@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_reference_loop_with_an_all_true_plan_is_the_plain_loop(tiny, sched):
    """with the oracle's own scheduler the plain loop is oracle.pipeline.tryon_pipeline; with the package's mirror it is the loop with every
    option off"""
    inp = _loop_inputs(tiny)
    a = (tiny["unet"], tiny["ucfg"], tiny["vae"], tiny["vcfg"], tiny["emasc"], inp)
    img_o, lat_o = P.tryon_pipeline(*a, num_inference_steps=4, guidance_scale=7.5, scheduler=sched)
    img0, lat0 = RT.tryon_reference(*a, 4, sched)
    n = 5 if sched == "pndm" else 4
    for interval in (None, 1, [1] * n):
        c = {}
        img, lat = _loop(tiny, inp, interval, steps=4, sched=sched, counts=c)
        assert torch.equal(lat, lat0) and torch.equal(img, img0)
        assert c["shallow"] == 0 and c["evals"] == n
        img, lat = _loop(tiny, inp, interval, steps=4, sched=P.make_scheduler(sched), counts=c)
        assert torch.equal(lat, lat_o) and torch.equal(img, img_o)
        assert c["shallow"] == 0 and c["evals"] == n


def test_reference_loop_counts_match_the_plan(tiny):
    import ladi_vton_amd as L
    inp = _loop_inputs(tiny)
    _, lat_plain = _loop(tiny, inp, None, steps=6)
    for interval, k in ((2, 0), (3, 1), ([1, 0, 0, 0, 1, 0], 2)):
        c = {}
        _, lat = _loop(tiny, inp, interval, k, steps=6, counts=c)
        flags = L.feature_cache_plan(6, interval)
        assert c["flags"] == flags and c["shallow"] == sum(1 for f in flags if not f) and c["cond_only"] == 0
        assert torch.isfinite(lat).all() and not torch.equal(lat, lat_plain)
    # under a guidance interval: the promoted plan, and the cond-only count of the schedule
    table = L.guidance_interval(6, 7.5, 0.3, 0.7)        # CFG on evaluations 2, 3, 4
    co = [not g > 1.0 for g in table]
    c = {}
    _, lat = _loop(tiny, inp, 3, 0, steps=6, table=table, counts=c)
    assert c["flags"] == L.feature_cache_plan(6, 3, co) == [True, False, True, True, False, False]
    assert c["shallow"] == 3 and c["cond_only"] == 3 and torch.isfinite(lat).all()
