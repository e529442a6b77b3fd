"""Token merging without a GPU: the host tables and merge counts of the library against tests/tome_ref.py, the configuration checks of
the C surface and of the Python layer, the PAG-overlap rule, and the reference against itself and against the oracle's transformer."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd import tome
from oracle import configs as C
from oracle import models as M
from tests import ref_unet as RU
from tests import tome_ref as R
from tests import util as U

SIZES = [(6, 8), (5, 7), (1, 9), (48, 64), (60, 80)]


def _tables(lib, h, w, use_rand, seed):
    T = h * w
    sp, dp = (ctypes.c_int * T)(), (ctypes.c_int * T)()
    nd = lib.ladi_tome_tables(h, w, 2, 2, use_rand, seed, sp, dp, T)
    assert nd >= 0, _lib.last_error()
    return list(sp[:T - nd]), list(dp[:nd])


@pytest.mark.parametrize("use_rand,seed", [(0, 0), (1, 3), (1, 2 ** 32 - 1)])
@pytest.mark.parametrize("h,w", SIZES)
def test_tables_match_the_reference(lib, h, w, use_rand, seed):
    sp, dp = _tables(lib, h, w, use_rand, seed)
    rs, rd = R.tables(h, w, 2, 2, bool(use_rand), seed)
    assert sp == rs and dp == rd
    assert len(dp) == (h // 2) * (w // 2) and sorted(sp + dp) == list(range(h * w))
    assert lib.ladi_tome_tables(h, w, 2, 2, use_rand, seed, None, None, 0) == len(dp)
    if not use_rand:
        assert all((p // w) % 2 == 0 and (p % w) % 2 == 0 for p in dp)


def test_random_tables_depend_on_the_seed(lib):
    a, b = _tables(lib, 48, 64, 1, 1)[1], _tables(lib, 48, 64, 1, 2)[1]
    assert a != b and a != _tables(lib, 48, 64, 0, 0)[1]
    offs = [((p // 64) % 2) * 2 + p % 2 for p in a]
    assert all(offs.count(o) > len(a) // 8 for o in range(4))          # every in-cell offset is drawn


def test_tables_refusals(lib):
    buf = (ctypes.c_int * 64)()
    assert lib.ladi_tome_tables(0, 8, 2, 2, 0, 0, None, None, 0) == -1 and "refused" in _lib.last_error()
    assert lib.ladi_tome_tables(6, 8, 3, 2, 0, 0, None, None, 0) == -1
    assert lib.ladi_tome_tables(6, 8, 2, 1, 0, 0, None, None, 0) == -1
    assert lib.ladi_tome_tables(6, 8, 2, 2, 0, 0, buf, buf, 35) == -1          # 36 src tokens
    assert lib.ladi_tome_tables(6, 8, 2, 2, 0, 0, buf, None, 64) == -1


@pytest.mark.parametrize("h,w", SIZES)
def test_merge_count(lib, h, w):
    T = h * w
    Ns = T - (h // 2) * (w // 2)
    for ratio in (0.0, 1.0 / T, 0.3, 0.5, 0.75, 0.99):
        assert lib.ladi_tome_merge_count(T, Ns, ratio) == R.merge_count(T, Ns, ratio) == min(int(T * ratio), Ns)
    assert lib.ladi_tome_merge_count(T, Ns, 0.0) == 0 and lib.ladi_tome_merge_count(T, Ns, 1.0 / T) in (0, 1)
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        assert lib.ladi_tome_merge_count(T, Ns, bad) == -1


GOOD = dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=0, seed=0, merge_attn=1, merge_crossattn=0, merge_mlp=0)
BAD = [(dict(ratio=1.0), "ratio"), (dict(ratio=-0.25), "ratio"), (dict(ratio=float("nan")), "ratio"), (dict(ratio=float("inf")), "ratio"),
       (dict(sx=4), "2 x 2"), (dict(sy=1), "2 x 2"), (dict(max_downsample=0), "max_downsample"), (dict(max_downsample=3), "max_downsample"),
       (dict(merge_attn=0), "all off")]


@pytest.mark.parametrize("over,word", BAD)
def test_config_refusals(lib, over, word):
    """every refusal of the C surface has a message, and the Python layer raises ValueError for the same configuration"""
    kw = dict(GOOD, **over)
    assert lib.ladi_tome_config_check(ctypes.byref(_lib.ToMeConfig(**kw))) == -1
    assert word in _lib.last_error(), _lib.last_error()
    with pytest.raises(ValueError):
        tome.config(**{k: (bool(v) if k.startswith("merge") or k == "use_rand" else v) for k, v in kw.items()})


def test_config_round_trip(lib):
    assert lib.ladi_tome_config_check(ctypes.byref(_lib.ToMeConfig(**GOOD))) == 0
    assert lib.ladi_tome_config_check(ctypes.byref(_lib.ToMeConfig(**dict(GOOD, ratio=0.0, merge_attn=0)))) == 0      # ratio 0 is off
    assert lib.ladi_tome_config_check(None) == -1
    assert tome.config() == dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False,
                                 merge_mlp=False)
    c = tome.config(0.25, max_downsample=2, use_rand=True, seed=7, merge_attn=False, merge_mlp=True)
    assert _lib.ToMeConfig(**{k: int(v) if isinstance(v, bool) else v for k, v in c.items()}).ratio == 0.25
    assert tuple(tome.FIELDS) == tuple(n for n, _ in _lib.ToMeConfig._fields_)
    for bad in (dict(seed=-1), dict(seed=2 ** 32), dict(ratio="0.5"), dict(ratio=True)):
        with pytest.raises(ValueError):
            tome.config(**bad)


def test_merged_blocks_and_the_pag_overlap_rule():
    from ladi_vton_amd.pipeline import pag_layer_mask
    pre = RU.block_prefixes(2)
    for md in (1, 2):
        assert [pre[b] for b in tome.merged_blocks(md, 2)] == RU.merged_prefixes(dict(max_downsample=md), 2)
    assert tome.merged_blocks(1, 2) == [0, 1, 13, 14, 15]
    cfg = tome.config(0.5)
    tome.check_pag_layers(cfg, pag_layer_mask("mid", 2), 2)                              # the default layer is fine
    tome.check_pag_layers(cfg, pag_layer_mask(["down.block_1", "up.block_2"], 2), 2)
    tome.check_pag_layers(tome.config(0.0), pag_layer_mask("down", 2), 2)                # off: nothing merges
    tome.check_pag_layers(None, pag_layer_mask("down", 2), 2)
    with pytest.raises(ValueError, match="merge tokens"):
        tome.check_pag_layers(cfg, pag_layer_mask("down.block_0", 2), 2)
    with pytest.raises(ValueError, match="merge tokens"):
        tome.check_pag_layers(tome.config(0.5, max_downsample=2), pag_layer_mask(["down.block_1", "up.block_2"], 2), 2)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def _case(h, w, Cc, ratio, seed=0, use_rand=False):
    g = torch.Generator().manual_seed(5 + h * w)
    x = torch.randn((h * w, Cc), generator=g, dtype=torch.float64)
    sp, dp = R.tables(h, w, 2, 2, use_rand, seed)
    return x, sp, dp, R.merge_count(h * w, len(sp), ratio)


@pytest.mark.parametrize("h,w,ratio", [(6, 8, 0.5), (5, 7, 0.3), (6, 8, 0.75), (12, 16, 0.99)])
def test_reference_unmerge_of_merge(h, w, ratio):
    x, sp, dp, r = _case(h, w, 16, ratio, 3, True)
    p = R.plan_of_metric(x, sp, dp, r)
    y = R.merge(x, p)
    back = R.unmerge(y, p)
    assert y.shape[0] == h * w - r and p["r"] == r and p["Nu"] == len(sp) - r
    kept = torch.tensor(p["unm"] + [p["dst"][j] for j, s in enumerate(p["segs"]) if not s], dtype=torch.long)
    assert torch.equal(back[kept], x[kept])                                   # tokens that took part in no merge come back exactly
    for j, s in enumerate(p["segs"]):
        if s:
            ref = x[[p["dst"][j]] + s].mean(dim=0)
            assert torch.allclose(back[p["dst"][j]], ref, rtol=1e-12, atol=1e-12) and all(torch.equal(back[q], back[p["dst"][j]]) for q in s)
    assert sum(len(s) for s in p["segs"]) == r
    q = R.plan_from_out_row(p["out_row"], sp, dp)
    assert q["unm"] == p["unm"] and q["segs"] == p["segs"] and R.plan_diff(p, q) == 0.0


def test_reference_ratio_zero_is_the_identity():
    x, sp, dp, r = _case(6, 8, 16, 0.0)
    assert r == 0
    p = R.plan_of_metric(x, sp, dp, 0)
    y = R.merge(x, p)
    assert torch.equal(R.unmerge(y, p), x) and sorted(p["unm"] + p["dst"]) == list(range(48))


def test_reference_select_ties_and_nan():
    sc = torch.tensor([0.5, 0.9, 0.5, float("nan"), 0.5, -0.0, 0.0, 0.9])
    assert R.select(sc, 3).tolist() == [True, True, False, False, False, False, False, True]
    assert R.select(sc, 4).tolist() == [True, True, True, False, False, False, False, True]
    assert R.select(sc, 6).tolist() == [True, True, True, False, True, True, False, True]      # -0 ties with +0: the lower index
    assert R.select(sc, 8).all()
    S = torch.tensor([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]])
    assert R.match(S)[1].tolist() == [1, 0]


def test_block_with_nothing_merged_is_the_oracle_block():
    """the block formula with the plan forced to "nothing merged" (a permutation: unmerged src, then dst) equals oracle.models.transformer2d"""
    torch.set_num_threads(U.cpu_quota_threads())
    cfg = C.UNET_TINY
    sd = {k: v.double() for k, v in C.synth_state_dict(C.unet_shapes(cfg), "unet.").items()}
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 64, 6, 8), generator=g, dtype=torch.float64)
    ehs = torch.randn((2, 8, cfg["cross_attention_dim"]), generator=g, dtype=torch.float64)
    p = "down_blocks.0.attentions.0"
    ref = M.transformer2d(sd, p, x, ehs, cfg["num_heads"][0], cfg["norm_num_groups"])
    sp, dp = R.tables(6, 8)
    none = R.make_plan(torch.zeros(len(sp), dtype=torch.bool), torch.zeros(len(sp), dtype=torch.long), sp, dp)
    for flags in (dict(merge_attn=True, merge_crossattn=False, merge_mlp=False), dict(merge_attn=True, merge_crossattn=True, merge_mlp=True)):
        tc = dict(ratio=0.5, max_downsample=1, use_rand=False, seed=0, **flags)
        got = RU.transformer2d(sd, p, x, ehs, cfg["num_heads"][0], cfg["norm_num_groups"], tome=(tc, [none, none], None, "proj_in"))
        assert U.rel_l2(got, ref) < 1e-12
        on = RU.transformer2d(sd, p, x, ehs, cfg["num_heads"][0], cfg["norm_num_groups"], tome=(tc, None, None, "proj_in"))
        assert U.rel_l2(on, ref) > 1e-4                                      # and merging is visible
    assert torch.equal(RU.transformer2d(sd, p, x, ehs, cfg["num_heads"][0], cfg["norm_num_groups"]), ref)
