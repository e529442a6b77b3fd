"""Host side of the fp16 range probe: the C ABI surface (header <-> ctypes), the RangeProbe report on injected values, and the point
enumeration for the released configuration.  No GPU."""
import os
import re

from ladi_vton_amd import _lib, configs
from ladi_vton_amd import probe as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ladi_probe_read_rank", "ladi_probe_create", "ladi_probe_destroy", "ladi_unet_attach_probe", "ladi_vae_attach_probe", "ladi_emasc_attach_probe",
           "ladi_probe_count", "ladi_probe_name", "ladi_probe_read", "ladi_probe_reset", "ladi_op_absmax"]


def test_header_declares_the_probe_abi_and_ctypes_binds_it_with_matching_arity():
    hdr = open(os.path.join(ROOT, "include", "ladi_native.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+ladi_probe\s+ladi_probe\s*;", hdr)            # the eleventh name: the handle type
    for name in SYMBOLS:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(args), (name, args)
    assert _lib.SIGNATURES["ladi_probe_name"][0] is _lib.c_char_p and _lib.SIGNATURES["ladi_probe_destroy"][0] is None


def test_library_exports_the_probe_symbols(lib):
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.ladi_probe_count(None) == -1 and lib.ladi_probe_name(None, 0) is None
    assert lib.ladi_unet_attach_probe(None, None) != 0


def _injected(names, absmax, nonfinite, rank=None):
    p = PR.RangeProbe.__new__(PR.RangeProbe)          # no device: the values a read would return are injected
    order, k = [], 0                                   # rank in time: by default the order of the points
    for c in nonfinite:
        k += 1 if c else 0
        order.append(k if c else 0)
    p._read = lambda: (list(names), list(absmax), list(nonfinite), list(rank or order))
    return p


def test_report_format_and_first_nonfinite_order():
    p = _injected(["conv_in", "down_blocks.0.resnets.0", "mid_block.attentions.0", "conv_out"], [2.0, 65504.0, 100.0, 0.0], [0, 0, 7, 12])
    rep = p.report()
    assert rep == [("conv_in", 2.0, 2.0 / 65504.0, 0), ("down_blocks.0.resnets.0", 65504.0, 1.0, 0), ("mid_block.attentions.0", 100.0, 100.0 / 65504.0, 7),
                   ("conv_out", 0.0, 0.0, 12)]
    assert p.first_nonfinite() == "mid_block.attentions.0"           # execution order, not magnitude or count
    # over a denoising loop the first in TIME wins: the NaNs of evaluation 0 reach conv_in (rank 3) only at evaluation 1
    loop = _injected(["conv_in", "mid_block.attentions.0", "conv_out"], [1.0, 1.0, 0.0], [5, 7, 12], rank=[3, 1, 2])
    assert loop.first_nonfinite() == "mid_block.attentions.0"
    assert _injected(["a", "b"], [1.0, 2.0], [0, 0]).first_nonfinite() is None
    assert _injected([], [], []).report() == [] and _injected([], [], []).first_nonfinite() is None
    lines = PR.RangeProbe.format(rep).splitlines()
    assert lines[0].split() == ["point", "absmax", "of", "65504", "nonfinite"] and len(lines) == 5
    # least head-room first: points that held inf / NaN, then by magnitude
    assert [ln.split()[0] for ln in lines[1:]] == ["mid_block.attentions.0", "conv_out", "down_blocks.0.resnets.0", "conv_in"]
    assert "100.0000%" in lines[3] and lines[1].split()[-1] == "7"
    assert [ln.split()[0] for ln in PR.RangeProbe.format(rep, sort_by_headroom=False).splitlines()[1:]] == [r[0] for r in rep]


def test_point_enumeration_of_the_released_configuration():
    cfg = configs.UNET_FULL
    L = cfg["layers_per_block"]
    names = PR.unet_point_names(cfg)
    # conv_in + down (4L resnets, 3L transformers, 3 samplers) + mid 3 + up (4(L+1) resnets, 3(L+1) transformers, 3 samplers) + conv_out
    assert len(names) == 1 + (4 * L + 3 * L + 3) + 3 + (4 * (L + 1) + 3 * (L + 1) + 3) + 1 == 46 and len(set(names)) == len(names)
    assert names[0] == "conv_in" and names[-1] == "conv_out" and names[1:3] == ["down_blocks.0.resnets.0", "down_blocks.0.attentions.0"]
    assert "down_blocks.3.attentions.0" not in names and "up_blocks.0.attentions.0" not in names and "up_blocks.3.upsamplers.0" not in names
    # every UNet name is the prefix of keys of the released state_dict layout
    keys = list(configs.unet_shapes(cfg))
    for n in names:
        assert any(k.startswith(n + ".") for k in keys), n
    vkeys = list(configs.vae_shapes(configs.VAE_FULL))
    enc, dec = PR.vae_encoder_point_names(), PR.vae_decoder_point_names()
    assert len(enc) == 7 and len(dec) == 7 and not set(enc) & set(dec) and not (set(enc) | set(dec)) & set(names)
    for n in enc + dec:
        assert any(k.startswith(n + ".") for k in vkeys), n
    em = PR.emasc_point_names(configs.EMASC_FULL)
    assert em == ["emasc.%d" % i for i in range(5)]
    total = len(enc) + len(em) + len(names) + len(dec)
    assert total == 65 and total <= 512                               # the default RangeProbe(max_points=512) holds a whole pipeline
