"""tools/range_report.py without a GPU: its arguments (defaults per --size, what it refuses) and the text it prints for a report."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("range_report_tool", os.path.join(ROOT, "tools", "range_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_follow_the_size(tool):
    a = tool.parse_args([])
    assert (a.size, a.height, a.width, a.tokens, a.batch, a.steps, a.checkpoint_dir) == ("full", 512, 384, 77, 1, 10, None)
    t = tool.parse_args(["--size", "tiny", "--steps", "3"])
    assert (t.height, t.width, t.tokens, t.steps) == (128, 128, 8, 3) and not t.execution_order
    o = tool.parse_args(["--size", "tiny", "--height", "64", "--tokens", "5", "--execution-order"])
    assert (o.height, o.width, o.tokens, o.execution_order) == (64, 128, 5, True)


@pytest.mark.parametrize("argv", [["--height", "100"], ["--width", "0"], ["--steps", "0"], ["--batch", "0"], ["--size", "small"],
                                  ["--checkpoint-dir", "x", "--size", "tiny"]])
def test_bad_arguments_are_refused(tool, argv):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(argv)
    assert e.value.code == 2


def test_rendered_table(tool):
    rep = [("conv_in", 2.0, 2.0 / 65504.0, 0), ("mid_block.attentions.0", 100.0, 100.0 / 65504.0, 7), ("conv_out", 300.0, 300.0 / 65504.0, 0)]
    lines = tool.render(rep, "mid_block.attentions.0").splitlines()
    assert [ln.split()[0] for ln in lines[1:4]] == ["mid_block.attentions.0", "conv_out", "conv_in"]          # least head-room first
    assert lines[4] == "" and lines[5] == "first non-finite activation: mid_block.attentions.0"
    lines = tool.render(rep, None, execution_order=True).splitlines()
    assert [ln.split()[0] for ln in lines[1:4]] == [r[0] for r in rep] and lines[-1] == "first non-finite activation: none"


def test_attach_only_follows_the_given_modules():
    """RangeProbe.attach_only (what the pipeline calls at the start of every run): detaches what is no longer listed, attaches what is new,
    leaves the rest alone -- on stand-in modules, with the library's attach call recorded"""
    from ladi_vton_amd import probe as PR

    class Mod:
        def __init__(self, name):
            self.h = name

    calls = []
    p = PR.RangeProbe.__new__(PR.RangeProbe)
    p.lib, p.h, p._attached = None, "probe", []
    p._attach_fn = lambda lib, m: (lambda mh, ph: calls.append((mh, ph)) or 0)
    u, v, e, v2 = Mod("u"), Mod("v"), Mod("e"), Mod("v2")
    assert p.attach_only(u, v, None) is p and calls == [("u", "probe"), ("v", "probe")] and p._attached == [u, v]
    del calls[:]
    p.attach_only(u, v, None)
    assert calls == [] and p._attached == [u, v]                      # nothing changed: nothing is called
    p.attach_only(u, v2, e)
    assert calls == [("v", None), ("v2", "probe"), ("e", "probe")] and p._attached == [u, v2, e]
    del calls[:]
    p.detach()
    assert calls == [("u", None), ("v2", None), ("e", None)] and p._attached == []
    p.h = None                                                        # (nothing for __del__ to destroy)
