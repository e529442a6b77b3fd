"""Any latent size on the host (no GPU): the reference forward in tests/ref_unet.py is oracle.models.unet_forward bit for bit wherever diffusers
does not set `forward_upsample_size`, it stretches to the skips' sizes where it does, and its statement of the nearest-index rule (the one
the igemm gather implements) is F.interpolate(size=..., mode="nearest")."""
import pytest
import torch
import torch.nn.functional as F

from oracle import configs as C
from oracle import models as M
from tests import ref_unet as R


@pytest.fixture(scope="module")
def tiny_unet():
    ucfg = C.UNET_TINY
    return ucfg, C.synth_state_dict(C.unet_shapes(ucfg), "unet.")


def _inputs(ucfg, n, h, w, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, ucfg["in_channels"], h, w), generator=g)
    ehs = torch.randn((n, 8, ucfg["cross_attention_dim"]), generator=g)
    return x, ehs


@pytest.mark.parametrize("hw", [(16, 16), (24, 16), (8, 8)])
def test_restatement_is_the_oracle_at_multiples_of_8(tiny_unet, hw):
    ucfg, sd = tiny_unet
    x, ehs = _inputs(ucfg, 2, *hw)
    ref, probe_ref = M.unet_forward(sd, ucfg, x, 481, ehs, return_probe=True)
    seen = {}
    got = R.unet_forward(sd, ucfg, x, 481, ehs, observe=seen.__setitem__)
    assert torch.equal(got, ref) and torch.equal(seen["mid_block.resnets.1"], probe_ref)
    tome0 = dict(ratio=0.0, max_downsample=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=True, merge_mlp=True)
    assert torch.equal(R.unet_forward(sd, ucfg, x, 481, ehs, tome=(tome0, None, None, "proj_in")), ref)           # token merging at ratio 0


@pytest.mark.parametrize("hw", [(17, 15), (9, 7), (12, 16)])
def test_restatement_keeps_the_latent_size_elsewhere(tiny_unet, hw):
    """at latents that are not multiples of 8 the oracle cannot even run (the doubled level and its skip differ in size); the restatement
    returns eps at the latent's size"""
    ucfg, sd = tiny_unet
    x, ehs = _inputs(ucfg, 1, *hw)
    with pytest.raises(RuntimeError):
        M.unet_forward(sd, ucfg, x, 481, ehs)
    got = R.unet_forward(sd, ucfg, x, 481, ehs)
    assert got.shape == (1, ucfg["out_channels"]) + hw and torch.isfinite(got).all()


def test_nearest_index_rule_matches_interpolate():
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 81)] + [(60, 120), (30, 60), (15, 30), (8, 15), (7, 15), (20, 40), (40, 80),
                                                                      (13, 25), (97, 193), (100, 199), (333, 667), (48, 96)]
    for n_in, n_out in pairs:
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        got = F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(-1).long().tolist()
        assert got == [R.nearest_src(d, n_in, n_out) for d in range(n_out)], (n_in, n_out)
