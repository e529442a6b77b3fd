"""Perturbed-attention guidance without a GPU: the reference forward against the oracle's (off: the same bits; on: visible at the parity
threshold the GPU tests use), the layer names and the per-evaluation scales of the pipeline against the reference's own, the C surface and
the pipeline's argument checks."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from oracle import configs as C
from oracle import models as M
from tests import pag_ref as R
from tests import ref_unet as RU
from tests import util as U


@pytest.fixture(scope="module")
def tiny():
    torch.set_num_threads(U.cpu_quota_threads())
    cfg = C.UNET_TINY
    sd = C.synth_state_dict(C.unet_shapes(cfg), "unet.")
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 31, 16, 8), generator=g).half().float()
    ehs = torch.randn((2, 8, cfg["cross_attention_dim"]), generator=g).half().float()
    return dict(cfg=cfg, sd=sd, x=torch.cat([x, x]), ehs=torch.cat([ehs, ehs]))


def test_reference_off_is_the_oracle_forward(tiny):
    plain = M.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"])
    assert torch.equal(RU.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"]), plain)
    every = set(RU.block_prefixes(2))
    assert torch.equal(RU.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"], pag=(every, None)), plain)
    assert torch.equal(RU.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"], pag=(every, 4)), plain)
    assert torch.equal(RU.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"], pag=((), 2)), plain)


@pytest.mark.parametrize("names", ["mid", ["down.block_0.attentions_1", "up.block_3"], ["down.block_1", "up.block_2"], ["down", "mid", "up"]])
def test_reference_perturbs_only_the_samples_from_pag_first(tiny, names):
    """samples 2, 3 are copies of 0, 1: with pag_first = 2 the first two keep the plain forward's bits and the last two are another function
    of the same inputs (below the 55 dB of the GPU forward test)"""
    plain = M.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"])
    out = RU.unet_forward(tiny["sd"], tiny["cfg"], tiny["x"], 481, tiny["ehs"], pag=(R.layer_prefixes(names), 2))
    p = U.psnr(out[2:], plain[2:])
    print("%s: perturbed samples %.1f dB from plain" % (names, p))
    assert torch.allclose(out[:2], plain[:2], rtol=0, atol=1e-5)
    assert p < 55.0, p


ACCEPTED = {
    "mid": [6], "down": [0, 1, 2, 3, 4, 5], "up": list(range(7, 16)),
    "down.block_0": [0, 1], "down.block_1": [2, 3], "down.block_2": [4, 5],
    "up.block_1": [7, 8, 9], "up.block_2": [10, 11, 12], "up.block_3": [13, 14, 15],
    "down.block_0.attentions_0": [0], "down.block_0.attentions_1": [1], "down.block_1.attentions_0": [2], "down.block_1.attentions_1": [3],
    "down.block_2.attentions_0": [4], "down.block_2.attentions_1": [5],
    "up.block_1.attentions_0": [7], "up.block_1.attentions_1": [8], "up.block_1.attentions_2": [9],
    "up.block_2.attentions_0": [10], "up.block_2.attentions_1": [11], "up.block_2.attentions_2": [12],
    "up.block_3.attentions_0": [13], "up.block_3.attentions_1": [14], "up.block_3.attentions_2": [15],
}
REJECTED = ["", "middle", "mid.block_0", "down.block_3", "up.block_0", "down.block_4", "up.block_4", "down.block_0.attentions_2",
            "up.block_1.attentions_3", "down.block_x", "down.block_0.resnets_0", "down.block_0.attentions_0.x", "side", "down.block_-1",
            "down_blocks.0", 3, None]


def test_pag_layer_mask():
    from ladi_vton_amd.pipeline import pag_layer_mask
    for name, bits in ACCEPTED.items():
        want = sum(1 << b for b in bits)
        assert pag_layer_mask(name, 2) == want == pag_layer_mask([name], 2), name
        assert R.mask_of(R.layer_prefixes(name, 2), 2) == want, name          # and the reference's own reading of the name agrees
    assert pag_layer_mask("mid", 2) == 1 << 6
    assert pag_layer_mask("down.block_1", 2) == (1 << 2) | (1 << 3)
    assert pag_layer_mask(["up.block_3", "down.block_0.attentions_1"], 2) == (1 << 13) | (1 << 14) | (1 << 15) | (1 << 1)
    assert pag_layer_mask(["down", "mid", "up"], 2) == 0xFFFF
    assert pag_layer_mask(("mid", "mid"), 2) == 1 << 6
    assert pag_layer_mask("mid", 1) == 1 << 3 and pag_layer_mask("up", 1) == 0b1111110000
    for name in REJECTED:
        with pytest.raises(ValueError):
            pag_layer_mask(name, 2)
        with pytest.raises(ValueError):
            pag_layer_mask(["mid", name], 2)
    with pytest.raises(ValueError):
        pag_layer_mask([], 2)


def test_pag_plan():
    import ladi_vton_amd as L
    from ladi_vton_amd.pipeline import pag_plan
    sch = L.DDIMScheduler()
    sch.set_timesteps(4)
    plan = pag_plan(3.0, 0.005, sch.timesteps)
    assert len(plan) == 4 and plan[0] > plan[1] > 0.0 and plan[2] == plan[3] == 0.0, plan
    assert plan == R.pag_plan(3.0, 0.005, sch.timesteps)
    assert plan[0] == pytest.approx(3.0 - 0.005 * (1000 - float(sch.timesteps[0])))
    assert pag_plan(3.0, 0.0, sch.timesteps) == [3.0] * 4 == R.pag_plan(3.0, 0.0, sch.timesteps)
    assert pag_plan(0.0, 0.0, sch.timesteps) == [0.0] * 4
    pn = L.PNDMScheduler()
    pn.set_timesteps(4)
    assert len(pag_plan(3.0, 0.0, pn.timesteps)) == 5 == len(pn.timesteps)
    for bad in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (3.0, -0.1), (3.0, float("nan")), ("x", 0.0)):
        with pytest.raises(ValueError):
            pag_plan(bad[0], bad[1], sch.timesteps)


def test_reference_combine():
    g = torch.Generator().manual_seed(3)
    u, c, p = (torch.randn((2, 4, 3, 3), generator=g, dtype=torch.float64) for _ in range(3))
    assert torch.equal(R.guided_eps(u, c, p, 7.5, 3.0), u + 7.5 * (c - u) + 3.0 * (c - p))
    assert torch.equal(R.guided_eps(None, c, p, 1.0, 3.0), c + 3.0 * (c - p))
    assert torch.equal(R.guided_eps(u, c, None, 7.5, 0.0), u + 7.5 * (c - u))
    e = u + 7.5 * (c - u) + 3.0 * (c - p)
    f = 0.7 * c.std(dim=[1, 2, 3], keepdim=True) / e.std(dim=[1, 2, 3], keepdim=True) + 0.3
    assert torch.allclose(R.guided_eps(u, c, p, 7.5, 3.0, 0.7), e * f, rtol=1e-12, atol=0)
    assert torch.equal(R.guided_eps(None, c, p, 1.0, 3.0, 0.7), c + 3.0 * (c - p))        # cond-only: no rescale


def test_c_surface():
    """the library exports the new symbols; the argument errors that need no device are raised with a message"""
    from ladi_vton_amd import _lib
    lib = _lib.load()
    for name in ("ladi_unet_pag_layer_count", "ladi_unet_set_pag_layers", "ladi_unet_pag_layers", "ladi_unet_forward_pag", "ladi_tryon_set_pag",
                 "ladi_op_pag_identity", "ladi_op_sched_run_pag", "ladi_op_cfg_stats_pag"):
        assert hasattr(lib, name), name
    assert lib.ladi_unet_pag_layer_count(None) == -1 and lib.ladi_unet_pag_layers(None) == 0
    assert lib.ladi_unet_set_pag_layers(None, 1 << 6) == -1 and "ladi_unet_set_pag_layers" in _lib.last_error()
    tab = (ctypes.c_float * 2)(3.0, 3.0)
    assert lib.ladi_tryon_set_pag(None, tab, 2) == -1 and "ladi_tryon_set_pag" in _lib.last_error()
    assert lib.ladi_unet_forward_pag(None, None, 0, 1, 1, 1, 1.0, None, 0, 0, 0, None) != 0 and "ladi_unet_forward_pag" in _lib.last_error()
    buf = (ctypes.c_uint16 * 64)()
    v = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ladi_op_pag_identity(None, 8, v, 8, 1, 8, None) != 0 and "null" in _lib.last_error()
    assert lib.ladi_op_pag_identity(v, 16, v, 16, 1, 12, None) != 0 and "C = 12" in _lib.last_error()
    assert lib.ladi_op_pag_identity(v, 8, v, 8, 0, 8, None) != 0 and "rows" in _lib.last_error()
    assert lib.ladi_op_pag_identity(v, 4, v, 8, 1, 8, None) != 0 and "stride" in _lib.last_error()
    assert lib.ladi_op_cfg_stats_pag(None, 4, 1, 4, 7.5, 3.0, 0.5, None, None) != 0
    assert lib.ladi_op_cfg_stats_pag(v, 4, 1, 4, 7.5, -1.0, 0.5, v, None) != 0 and "PAG scale" in _lib.last_error()
    assert lib.ladi_op_sched_run_pag(0, 2, None, 0.0, v, 4, 2, 1, 4, 1, tab, None, 0.0, v, None, 0, None) == -1
    assert "null PAG table" in _lib.last_error()
    bad = (ctypes.c_float * 2)(3.0, -1.0)
    assert lib.ladi_op_sched_run_pag(0, 2, None, 0.0, v, 4, 2, 1, 4, 1, tab, bad, 0.0, v, None, 0, None) != 0
    assert "PAG table entry" in _lib.last_error()


def _pipe(unet):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=[1, 2, 3, 4])), text_encoder=None,
                                           tokenizer=None, unet=unet, scheduler=L.DDIMScheduler())


def test_pipeline_misuse():
    class PlainUNet:
        config = SimpleNamespace(sample_size=8)

    pipe = _pipe(PlainUNet())
    with pytest.raises(ValueError, match="PlainUNet"):
        pipe.set_pag_applied_layers("mid")
    img, mask = torch.zeros((1, 3, 64, 64)), torch.zeros((1, 1, 64, 64))
    kw = dict(image=img, mask_image=mask, pose_map=None, warped_cloth=None, prompt_embeds=torch.zeros((1, 8, 4)), num_inference_steps=4)
    with pytest.raises(ValueError, match="`pag_scale` needs the native UNet \\(NativeUNet\\), the pipeline holds PlainUNet"):
        pipe(pag_scale=3.0, **kw)
    for ps, pa in ((-1.0, 0.0), (float("nan"), 0.0), (3.0, -0.5), (3.0, float("inf"))):
        with pytest.raises(ValueError, match="pag_"):
            pipe(pag_scale=ps, pag_adaptive_scale=pa, **kw)
    calls = []
    pipe = _pipe(SimpleNamespace(config=SimpleNamespace(sample_size=8), set_pag_applied_layers=calls.append))
    pipe.set_pag_applied_layers(["down.block_1", "up.block_2"])
    assert calls == [["down.block_1", "up.block_2"]]
    with pytest.raises(ValueError, match="feature_cache"):
        pipe(pag_scale=3.0, feature_cache=2, **kw)
    with pytest.raises(ValueError, match="feature_cache"):
        pipe(pag_scale=3.0, feature_cache={"interval": 2, "branch": 1}, **kw)
