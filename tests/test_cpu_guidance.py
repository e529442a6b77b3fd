"""Guidance schedule, CFG cut-off and guidance rescale, host side: the reference loop (tests/ref_tryon.py) is pinned to the
oracle pipeline before anything is compared with it; the guidance_interval helper; the Python-side validation; the ABI declarations."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from oracle import configs as C
from oracle import pipeline as P
from tests import guidance_ref as G
from tests import ip_adapter_ref as IP
from tests import ref_tryon as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ladi_tryon_set_guidance_schedule", "ladi_tryon_set_guidance_rescale", "ladi_tryon_cond_only_evals", "ladi_op_sched_run_guided",
               "ladi_op_cfg_stats"]


@pytest.fixture(scope="module")
def tiny():
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sd = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
              emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    inp = P.synthetic_inputs(1, 128, 128, L=8, D=ucfg["cross_attention_dim"])
    return dict(ucfg=ucfg, vcfg=vcfg, sd=sd, inp=inp)


def _counts(info):
    return {k: info[k] for k in ("full", "cond_only")}


@pytest.mark.parametrize("scheduler,steps,evals", [("ddim", 3, 3), ("pndm", 3, 4)])
@pytest.mark.parametrize("scale", [7.5, 1.0])
def test_reference_constant_schedule_is_the_oracle_pipeline(tiny, scheduler, steps, evals, scale):
    """tryon_reference with a constant schedule and phi = 0 IS oracle.pipeline.tryon_pipeline: equal, not close (scale 1.0: the run without
    CFG); the forward counts are what the schedule implies.  So is the loop with each feature at its off value"""
    a = (tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], tiny["inp"])
    ref_img, ref_lat = P.tryon_pipeline(*a, num_inference_steps=steps, guidance_scale=scale, scheduler=scheduler)
    counts = {}
    img, lat = RT.tryon_reference(*a, steps, P.make_scheduler(scheduler), table=[scale] * evals, info=counts)
    assert torch.equal(lat, ref_lat) and torch.equal(img, ref_img)
    assert _counts(counts) == (dict(full=evals, cond_only=0) if scale > 1 else dict(full=0, cond_only=evals))
    # every other option at its off value is that same run
    sd_ip = IP.make_adapter(tiny["ucfg"])
    tome0 = dict(ratio=0.0, max_downsample=1, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False, merge_mlp=False)
    off = dict(cache_none=dict(feature_cache=(None, 0)), cache_1=dict(feature_cache=(1, 0)), cache_flags=dict(feature_cache=([True] * evals, 1)),
               pag_0=dict(pag=(0.0, 0.0, ("mid",))), ip_zero=dict(ip=(sd_ip, torch.ones(1, 64), None, [0.0] * 16)), tome_0=dict(tome=(tome0, None)),
               preserve_none=dict(preserve=(None, 0.0)), first_step_0=dict(first_step=0, init_latents=torch.ones(1, 4, 16, 16)), freeu_none=dict(freeu=None))
    for name, kw in off.items():
        img, lat = RT.tryon_reference(*a, steps, P.make_scheduler(scheduler), table=[scale] * evals, **kw)
        assert torch.equal(lat, ref_lat) and torch.equal(img, ref_img), name


def test_reference_cut_off_and_rescale_change_the_result(tiny):
    """the restatement's two new branches do something: a cut-off run differs from the constant one and counts its cond-only forwards; phi
    rescales the guided prediction to the conditional one's standard deviation (phi = 1: equal stds)"""
    a = (tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], tiny["inp"])
    _, lat_c = RT.tryon_reference(*a, 3, P.make_scheduler("ddim"), table=[7.5] * 3)
    counts = {}
    _, lat_i = RT.tryon_reference(*a, 3, P.make_scheduler("ddim"), table=[7.5, 1.0, 7.5], info=counts)
    assert _counts(counts) == dict(full=2, cond_only=1) and not torch.equal(lat_c, lat_i)
    g = torch.Generator().manual_seed(3)
    eu, ec = torch.randn((3, 4, 5, 7), generator=g, dtype=torch.float64), torch.randn((3, 4, 5, 7), generator=g, dtype=torch.float64) * 0.5
    e1 = G.guided_eps(eu, ec, 7.5, 1.0)
    assert torch.allclose(e1.std(dim=[1, 2, 3]), ec.std(dim=[1, 2, 3]), rtol=1e-12)
    e0, e7 = G.guided_eps(eu, ec, 7.5, 0.0), G.guided_eps(eu, ec, 7.5, 0.7)
    f = 0.7 * ec.std(dim=[1, 2, 3]) / e0.std(dim=[1, 2, 3]) + 0.3
    assert torch.allclose(e7, e0 * f[:, None, None, None], rtol=1e-12)


def test_guidance_interval_edges():
    from ladi_vton_amd import guidance_interval
    assert guidance_interval(0, 7.5, 0.0, 1.0) == []
    assert guidance_interval(1, 7.5, 0.0, 1.0) == [7.5]
    assert guidance_interval(1, 7.5, 0.0, 0.0) == [1.0]
    assert guidance_interval(1, 7.5, 0.5, 1.0) == [1.0]           # ceil(0.5) = 1: the only evaluation lies before the interval
    assert guidance_interval(10, 7.5, 0.0, 0.6) == [7.5] * 6 + [1.0] * 4      # 0.6 * 10 lands on index 6: exclusive
    assert guidance_interval(10, 7.5, 0.2, 0.5) == [1.0] * 2 + [7.5] * 3 + [1.0] * 5
    assert guidance_interval(4, 5.0, 0.25, 0.75) == [1.0, 5.0, 5.0, 1.0]      # both ends land on an index
    assert guidance_interval(51, 7.5, 0.0, 0.6).count(7.5) == math.ceil(0.6 * 51) == 31
    assert guidance_interval(5, 3.0, 0.0, 1.0) == [3.0] * 5
    assert guidance_interval(5, 3.0, 1.0, 1.0) == [1.0] * 5
    with pytest.raises(ValueError):
        guidance_interval(5, 3.0, -0.1, 1.0)


def _stub_pipe(scheduler):
    import ladi_vton_amd as L
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=[1, 2, 3, 4], scaling_factor=0.18215))
    unet = SimpleNamespace(config=SimpleNamespace(sample_size=16))
    return L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=scheduler)


def test_python_side_validation():
    """every misuse is a ValueError raised before a device is touched (this test has none)"""
    import ladi_vton_amd as L
    from ladi_vton_amd.pipeline import guidance_plan
    img, mask = torch.zeros(1, 3, 128, 128), torch.zeros(1, 1, 128, 128)
    pe = torch.zeros(1, 8, 32)

    def call(pipe, **kw):
        return pipe(image=img, mask_image=mask, pose_map=torch.zeros(1, 18, 128, 128), warped_cloth=img, prompt_embeds=pe, height=128, width=128,
                    num_inference_steps=4, **kw)
    ddim, pndm = _stub_pipe(L.DDIMScheduler()), _stub_pipe(L.PNDMScheduler())
    with pytest.raises(ValueError, match="4 evaluations"):
        call(ddim, guidance_scale=[7.5] * 5, negative_prompt_embeds=pe)
    with pytest.raises(ValueError, match="5 evaluations"):             # PNDM: steps + 1
        call(pndm, guidance_scale=[7.5] * 4, negative_prompt_embeds=pe)
    with pytest.raises(ValueError, match="finite and >= 0"):
        call(ddim, guidance_scale=[7.5, -1.0, 7.5, 7.5], negative_prompt_embeds=pe)
    with pytest.raises(ValueError, match="finite and >= 0"):
        call(ddim, guidance_scale=[7.5, float("nan"), 7.5, 7.5], negative_prompt_embeds=pe)
    with pytest.raises(ValueError, match="finite and >= 0"):
        call(ddim, guidance_scale=lambda i, n: float("inf"), negative_prompt_embeds=pe)
    for phi in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            call(ddim, guidance_scale=7.5, negative_prompt_embeds=pe, guidance_rescale=phi)
    # any scale > 1 turns classifier-free guidance on, and _encode_prompt then asks for the negative embeddings as it does for a scalar > 1
    for gs in ([1.0, 1.0, 1.5, 1.0], lambda i, n: 2.0 if i == n - 1 else 0.0):
        do_cfg = guidance_plan(gs, 4)[2]
        assert do_cfg is True
        with pytest.raises(ValueError, match="negative_prompt_embeds"):
            ddim._encode_prompt(None, torch.device("cpu"), 1, do_cfg, prompt_embeds=pe)
    assert ddim._encode_prompt(None, torch.device("cpu"), 1, guidance_plan([1.0, 0.5, 0.0, 1.0], 4)[2], prompt_embeds=pe)[1] is None
    # what a valid argument resolves to
    assert guidance_plan(7.5, 4) == (None, 7.5, True) and guidance_plan(1.0, 4) == (None, 1.0, False)
    assert guidance_plan([1.0, 0.0, 0.5, 1.0], 4) == ([1.0, 0.0, 0.5, 1.0], 1.0, False)
    assert guidance_plan(lambda i, n: 7.5 if i < n // 2 else 1.0, 4, 0.7) == ([7.5, 7.5, 1.0, 1.0], 7.5, True)
    assert guidance_plan(torch.tensor(7.5), 4)[2] is True


def test_header_and_ctypes_declare_the_new_symbols():
    from ladi_vton_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ladi_native.h")).read()
    declared = set(re.findall(r"\b(ladi_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    # argument counts of the prototypes match the ctypes signatures
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
