"""LoRA without a GPU: the key normaliser (PEFT, legacy diffusers and kohya forms of one adapter give the same tensors; ambiguous '_' names;
prefixes; alpha; text-encoder keys; what raises), the reference helpers of tests/lora_ref.py against each other, and the C-ABI surface of the
new entry points on null handles and bad arguments."""
import ctypes
import warnings
from collections import OrderedDict

import pytest
import torch

from ladi_vton_amd import _lib, configs as C, lora
from tests import lora_ref as R

MODS = lora.target_modules(C.UNET_TINY)
SHAPES = {k[:-len(".weight")]: s for k, s in C.unet_shapes(C.UNET_TINY).items() if k.endswith(".weight") and len(s) >= 2}
XF = "down_blocks.0.attentions.1.transformer_blocks.0"
PICK = OrderedDict([(XF + ".attn1.to_q", 4), (XF + ".attn1.to_out.0", 7), (XF + ".attn2.to_k", 4), (XF + ".ff.net.0.proj", 7), (XF + ".ff.net.2", 4),
                    ("down_blocks.0.attentions.1.proj_in", 3), ("up_blocks.1.resnets.0.conv_shortcut", 4), ("down_blocks.1.resnets.0.conv1", 7),
                    ("mid_block.resnets.0.time_emb_proj", 4), ("down_blocks.0.downsamplers.0.conv", 5), ("conv_in", 4),
                    ("time_embedding.linear_1", 2)])


def _formats(ad):
    """the adapter `ad` (library keys) written as PEFT, legacy diffusers (module and attention-processor form) and kohya"""
    peft, legacy, kohya = OrderedDict(), OrderedDict(), OrderedDict()
    for m in PICK:
        down, up, alpha = R.adapter_factors(ad, m)
        up4 = up.reshape(up.shape[0], up.shape[1], 1, 1) if down.dim() == 4 else up
        peft["base_model.model.unet." + m + ".lora_A.weight"], peft["base_model.model.unet." + m + ".lora_B.weight"] = down, up4
        head, _, leaf = m.rpartition(".")
        if ".attn" in m and leaf in ("to_q", "to_k", "to_v"):
            legacy["unet.%s.processor.%s_lora.down.weight" % (head, leaf)], legacy["unet.%s.processor.%s_lora.up.weight" % (head, leaf)] = down, up
        elif m.endswith(".to_out.0"):
            a = m[:-len(".to_out.0")]
            legacy["unet.%s.processor.to_out_lora.down.weight" % a], legacy["unet.%s.processor.to_out_lora.up.weight" % a] = down, up
        else:
            legacy["unet." + m + ".lora.down.weight"], legacy["unet." + m + ".lora.up.weight"] = down, up4
        k = "lora_unet_" + m.replace(".", "_")
        kohya[k + ".lora_down.weight"], kohya[k + ".lora_up.weight"], kohya[k + ".alpha"] = down, up4, torch.tensor(alpha)
    return peft, legacy, kohya


def test_target_modules_cover_every_conv_and_linear():
    assert len(MODS) == len(set(MODS)) == 282
    for leaf in ("conv_in", "conv_out", "time_embedding.linear_2", "up_blocks.0.upsamplers.0.conv", XF + ".attn2.to_v", XF + ".ff.net.0.proj",
                 "mid_block.attentions.0.proj_out", "up_blocks.3.resnets.2.time_emb_proj"):
        assert leaf in MODS, leaf
    assert not [m for m in MODS if "norm" in m]


def test_three_formats_normalise_to_equal_tensors():
    ad = R.make_adapter(5, SHAPES, PICK)            # no alpha keys: alpha = rank
    want = lora.normalize_state_dict(ad, MODS)
    assert list(want) == list(PICK)
    for name, sd in zip(("peft", "legacy", "kohya"), _formats(ad)):
        got = lora.normalize_state_dict(sd, MODS)
        assert set(got) == set(PICK), name
        for m, r in PICK.items():
            (d0, u0, a0), (d1, u1, a1) = want[m], got[m]
            assert d1.dtype == u1.dtype == torch.float32
            assert torch.equal(d0, d1) and torch.equal(u0, u1) and a0 == a1 == float(r), (name, m)
            assert tuple(d1.shape) == (r,) + tuple(SHAPES[m][1:]) and tuple(u1.shape) == (SHAPES[m][0], r), (name, m)   # conv down stays 4-D
        assert got.text_encoder_keys == ()


def test_ambiguous_underscores_resolve_by_table():
    """to_out_0 / ff_net_0_proj / time_emb_proj / conv_shortcut: a split at every '_' would be wrong; the table built from the names is not"""
    for m in (XF + ".attn1.to_out.0", XF + ".ff.net.0.proj", XF + ".ff.net.2", "mid_block.resnets.0.time_emb_proj",
              "up_blocks.1.resnets.0.conv_shortcut", "time_embedding.linear_1", "down_blocks.0.downsamplers.0.conv"):
        ad = R.make_adapter(9, SHAPES, {m: 3}, alpha=1.5)
        k = "lora_unet_" + m.replace(".", "_")
        sd = {k + ".lora_down.weight": ad[m + ".lora_down.weight"], k + ".lora_up.weight": ad[m + ".lora_up.weight"], k + ".alpha": ad[m + ".alpha"]}
        got = lora.normalize_state_dict(sd, MODS)
        assert list(got) == [m] and got[m][2] == 1.5
    with pytest.raises(ValueError, match="names no conv"):
        lora.normalize_state_dict({"lora_unet_down_blocks_0_attentions_1_to_q.lora_down.weight": torch.zeros(2, 64)}, MODS)
    with pytest.raises(ValueError, match="collide"):
        lora.normalize_state_dict({}, ["a.b_c", "a_b.c"])


def test_prefixes_alpha_and_text_encoder_keys():
    m = XF + ".attn2.to_v"
    ad = R.make_adapter(3, SHAPES, {m: 4})
    d, u = ad[m + ".lora_down.weight"], ad[m + ".lora_up.weight"]
    for pre in ("", "unet.", "base_model.model.", "base_model.model.unet."):
        got = lora.normalize_state_dict({pre + m + ".lora_A.weight": d, pre + m + ".lora_B.weight": u}, MODS)
        assert list(got) == [m] and torch.equal(got[m][0], d) and got[m][2] == 4.0           # missing alpha: the rank
    got = lora.normalize_state_dict({m + ".lora_A.default_0.weight": d, m + ".lora_B.default_0.weight": u, m + ".alpha": torch.tensor(8.0)}, MODS)
    assert got[m][2] == 8.0
    te = {"lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8), "text_encoder.text_model.x.lora_A.weight": torch.zeros(4, 8),
          "lora_te1_text_model_y.alpha": torch.tensor(4.0)}
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = lora.normalize_state_dict(dict(te, **{"unet." + m + ".lora.down.weight": d, "unet." + m + ".lora.up.weight": u}), MODS)
    assert list(got) == [m] and set(got.text_encoder_keys) == set(te) and any("text-encoder" in str(w.message) for w in rec)
    flat = lora.to_library_keys(got)
    assert set(flat) == {m + ".lora_down.weight", m + ".lora_up.weight", m + ".alpha"} and float(flat[m + ".alpha"]) == 4.0


def test_what_raises():
    m = XF + ".attn1.to_q"
    ad = R.make_adapter(3, SHAPES, {m: 4})
    d, u = ad[m + ".lora_down.weight"], ad[m + ".lora_up.weight"]
    ok = {m + ".lora_A.weight": d, m + ".lora_B.weight": u}
    for extra, pat in (({m + ".lora_magnitude_vector.weight": torch.zeros(64)}, "DoRA"), ({"lora_unet_x.dora_scale": torch.zeros(64)}, "DoRA"),
                       ({m + ".lora_B.bias": torch.zeros(64)}, "bias"), ({m + ".bias": torch.zeros(64)}, "bias"),
                       ({"down_blocks.0.attentions.1.norm.lora_A.weight": d}, "not a conv / linear"),
                       ({"down_blocks.9.resnets.0.conv1.lora_A.weight": d}, "not a conv / linear"),
                       ({m + ".weight": d}, "not a LoRA factor")):
        with pytest.raises(ValueError, match=pat):
            lora.normalize_state_dict(dict(ok, **extra), MODS)
    with pytest.raises(ValueError, match="missing"):
        lora.normalize_state_dict({m + ".lora_A.weight": d}, MODS)
    with pytest.raises(ValueError, match="rank"):
        lora.normalize_state_dict({m + ".lora_A.weight": d, m + ".lora_B.weight": u[:, :3]}, MODS)
    with pytest.raises(ValueError, match="two down"):
        lora.normalize_state_dict(dict(ok, **{"unet." + m + ".lora.down.weight": d}), MODS)


def test_reference_maps_and_merge():
    """lora_ref against itself: pack / unpack are inverse under both row maps, the GEGLU map is load_geglu's, the merge is base + scale up down"""
    g = torch.Generator().manual_seed(1)
    assert R.geglu_rows(64).tolist()[:3] == [0, 1, 2] and R.geglu_rows(64).tolist()[32] == 64 and R.geglu_rows(64).tolist()[64] == 32
    assert sorted(R.geglu_rows(96).tolist()) == list(range(192))
    for shape, geglu, row0 in (((64, 31, 3, 3), False, 64), ((128, 64), True, 64), ((64, 64), False, 0)):
        w = torch.randn(shape, generator=g).half().float()
        taps = 9 if len(shape) == 4 else 1
        p = R.pack_rows(w, total_rows=shape[0] + 128, row0=row0, geglu=geglu, fill=7.0)
        assert p.shape == (shape[0] + 128, taps * R.pad64(shape[1]))
        assert torch.equal(R.unpack_rows(p, shape[0], shape[1], taps, row0, geglu), w.reshape(shape[0], shape[1], taps).double())
        assert float(p[:row0].min() if row0 else 7.0) == 7.0 and float(p[row0 + shape[0]:].min()) == 7.0
        if shape[1] == 31:
            assert not p.reshape(-1, taps, 64)[row0:row0 + 64, :, 31:].any()
    base = torch.randn((8, 5, 3, 3), generator=g)
    up, down = torch.randn((8, 2), generator=g), torch.randn((2, 5, 3, 3), generator=g)
    ref, mag, K = R.merge_ref(base, [(0.5, up, down), (2.0, up, down)])
    want = base.double() + 2.5 * torch.einsum("or,rikl->oikl", up.double(), down.double())
    assert K == 4 and torch.allclose(ref, want, rtol=1e-12, atol=1e-12) and bool((mag >= ref.abs() - 1e-12).all())
    assert R.fp32_scale(0.3, 4.0, 7) == float(torch.tensor(0.3 * 4.0 / 7, dtype=torch.float64).float())
    lim = R.merge_limit(ref, mag, K)
    assert bool((lim >= 0.5 * 2.0 ** -24).all()) and bool((lim <= 2.0 ** -10 * (ref.abs() + mag) + 2.0 ** -24).all())


# ---------------------------------------------------------------------------------------------------------------- C ABI, no device
def test_entry_points_refuse_null_handles_and_bad_arguments(lib):
    err = _lib.last_error
    names = (ctypes.c_char_p * 1)(b"a")
    ws = (ctypes.c_float * 1)(1.0)
    assert lib.ladi_unet_lora_load(None, b"a", None) != 0 and "ladi_unet_lora_load" in err() and "null" in err()
    assert lib.ladi_unet_set_adapters(None, names, ws, 1, None) != 0 and "ladi_unet_set_adapters" in err() and "null" in err()
    assert lib.ladi_unet_lora_delete(None, b"a") != 0 and "ladi_unet_lora_delete" in err()
    assert lib.ladi_unet_lora_count(None) == -1 and "ladi_unet_lora_count" in err()
    assert lib.ladi_unet_lora_name(None, 0) is None and "ladi_unet_lora_name" in err()
    assert lib.ladi_unet_lora_active(None, None, None, 0) == -1 and "ladi_unet_lora_active" in err()
    assert lib.ladi_unet_export_weight(None, b"conv_in.weight", None, 0) == -1 and "ladi_unet_export_weight" in err()
    # the operator: every refusal comes before anything is launched (the addresses below are never read)
    P = ctypes.c_void_p
    ups, dns = (P * 8)(*[0x2000] * 8), (P * 8)(*[0x3000] * 8)
    rk, sc = (ctypes.c_int * 8)(*[4] * 8), (ctypes.c_float * 8)(*[1.0] * 8)

    def op(base=0x10000, W=0x20000, pitch=64, cin=64, cin_pad=64, taps=1, row0=0, rows=64, half=0, n=1, up=ups, down=dns, rank=rk, scale=sc):
        return lib.ladi_op_lora_merge(base, W, pitch, cin, cin_pad, taps, row0, rows, half, n, up, down, rank, scale, None, None)

    for kw, pat in ((dict(base=None), "null"), (dict(W=None), "null"), (dict(W=0x10000), "base == W"), (dict(n=9), "n_adapters"), (dict(n=-1), "n_adapters"),
                    (dict(up=None), "null up"), (dict(rows=0), "size"), (dict(cin=0), "size"), (dict(cin=65), "cin_pad"), (dict(cin_pad=96, pitch=96), "multiple of 64"),
                    (dict(pitch=32), "pitch"), (dict(pitch=68), "pitch"), (dict(base=0x10008), "aligned"), (dict(W=0x20002), "aligned"),
                    (dict(taps=9), "pitch"), (dict(row0=-1), "size"), (dict(half=16, rows=32), "GEGLU"), (dict(half=32, rows=96), "GEGLU"),
                    (dict(half=32, row0=32), "GEGLU"), (dict(rank=(ctypes.c_int * 8)(*[0] * 8)), "rank"), (dict(rank=(ctypes.c_int * 8)(*[257] * 8)), "rank"),
                    (dict(up=(P * 8)(*[0] * 8)), "factor"), (dict(scale=(ctypes.c_float * 8)(*[float("nan")] * 8)), "finite")):
        assert op(**kw) != 0, kw
        assert "ladi_op_lora_merge" in err() and pat in err(), (kw, err())
