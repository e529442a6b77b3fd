"""The tile selections production runs, element by element against float64, and the selection path itself.

tests/golden/igemm_product_launches.txt lists the distinct implicit-GEMM launches of the product (tools/dump_igemm_launches.py).  Every
distinct record, reduced by tests/tuned_cases.py to the smallest problem that still takes the production launch's code path, is launched
with the recorded configuration and judged with check_elem against the float64 reference of tests/util.py between poison rows; the
conditions of the reduction are asserted on what the launch itself reports (ladi_igemm_last_launch, stats_row_px).  Nothing is timed
inside a test: the tuner is off wherever a launch could otherwise measure."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from tests import tuned_cases as T
from tests import util as U

pytestmark = pytest.mark.gpu

REDUCED = T.reduced_records()
GEOMS = sorted({T.geometry_id(q): q for q in REDUCED}.items())          # one representative record per distinct reduced geometry
SHIPPED = {tuple(row[:8]): row[8] for row in T.parse_table()}
# records that are small at full size and that the SHIPPED table serves (a source-1 record of a later capture run may be served by an earlier
# run's measurement instead)
SMALL = [r for r in T.golden_records() if SHIPPED.get(tuple(r["key"])) == r["cfg"] and r["P"] <= 2048 and T.ref_flop(r) <= T.REF_FLOP_LIMIT]


def _record(key, value):
    U.record_parity("tuned/" + key, value)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


@pytest.fixture
def tuner_off(lib):
    lib.ladi_igemm_set_autotune(0)
    yield
    lib.ladi_igemm_set_autotune(1)


def _launch(pb, lib, cfg):
    """pb.launch; a HIP error (a fault surfaces at the synchronize) ends the session: nothing further is started on a device that faulted"""
    try:
        return pb.launch(lib, cfg)
    except RuntimeError as e:
        q = pb.q
        pytest.exit("HIP error in P=%d Q=%d K=%d ksize=%d ops=%d cfg %d: %s" % (q["P"], q["Q"], q["K"], q["ksize"], q["opmask"], cfg, e), returncode=3)


def _launched(res):
    return res["last"][1] & 15, res["last"][1] >> 4, res["last"][2], res["px"]


# ---------------------------------------------------------------------------------------------------------------------- shipped selections
@pytest.mark.parametrize("i", range(len(REDUCED)), ids=[T.name_of(q) for q in REDUCED])
def test_shipped_selection_against_float64(lib, i):
    """the reduced problem of one production record with the recorded configuration given explicitly: accepted, inside the per-element bound,
    guards untouched, statistics rows judged; and the reduction kept the kernel family, the tile map kind (G > 1 for kind 3), the split-K
    factor, stats_row_px, two samples and two pixel tiles per sample wherever production had them -- read back from the launch"""
    q = REDUCED[i]
    pb = T.problem(q)
    res = _launch(pb, lib, q["cfg"])
    what = "%s %s" % (T.name_of(q), res["last"])
    assert res["rc"] == 0, "%s: cfg %d refused the reduced launch: rc = %d (%s)" % (what, q["cfg"], res["rc"], _lib.last_error())
    assert res["sel"] == [q["cfg"], 0], res["sel"]
    assert res["last"][0] == q["last"][0], "%s: kernel family %d, production ran %d" % (what, res["last"][0], q["last"][0])
    bad = T.conditions(q, q, _launched(res))
    assert not bad, "%s: the reduced problem left production's code path: %s" % (what, bad)
    ratio, sratio = pb.judge(res, what)
    _record(T.name_of(q), dict(ratio=round(ratio, 4), family=T.FAMILY[res["last"][0]], P=q["P"], **({"stats": round(sratio, 4)} if sratio is not None else {})))
    assert ratio <= 1.0 and (sratio is None or sratio <= 1.0)


@pytest.mark.parametrize("i", range(len(GEOMS)), ids=[T.name_of(q) for _, q in GEOMS])
def test_cost_model_choice_is_admissible_and_right(lib, tuner_off, i):
    """tuner off: cfg = 0 on every distinct reduced problem launches something the admission rule accepts, and the output is inside the bound"""
    q = GEOMS[i][1]
    pb = T.problem(q)
    res = _launch(pb, lib, 0)
    what = "%s cost model %s" % (T.name_of(q), res["sel"])
    assert res["rc"] == 0, "%s: rc = %d (%s)" % (what, res["rc"], _lib.last_error())
    cfg, src = res["sel"]
    assert src in (3, 4) and 1 <= cfg <= lib.ladi_igemm_cfg_count(), res["sel"]
    assert lib.ladi_igemm_cfg_admissible(ctypes.byref(res["desc"]), q["batch"], cfg, 0) == 1, what
    ratio, _ = pb.judge(res, what)
    _record("cost_model/" + T.name_of(q), dict(ratio=round(ratio, 4), cfg=cfg))
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- the table serves
@pytest.mark.parametrize("i", range(len(SMALL)), ids=[T.name_of(r) for r in SMALL])
def test_table_lookup_serves_the_launch(lib, i):
    """records that are small at full size (the KV projections, the 8x6 level, the batched rows), launched with cfg = 0 at the real shape: the
    table's configuration is what runs, by source 1, and the output is right"""
    r = SMALL[i]
    assert lib.ladi_igemm_tune_lookup((ctypes.c_int * 8)(*r["key"])) == r["cfg"]          # a miss would make the launch below measure
    pb = T.problem(r)
    res = _launch(pb, lib, 0)
    what = "%s from the table %s" % (T.name_of(r), res["last"])
    assert res["rc"] == 0, "%s: rc = %d (%s)" % (what, res["rc"], _lib.last_error())
    assert res["sel"] == [r["cfg"], 1], "%s: launched %s, the table holds cfg %d" % (what, res["sel"], r["cfg"])
    assert res["last"] == r["last"] and res["px"] == r["px"], (what, r["last"], res["px"], r["px"])
    ratio, sratio = pb.judge(res, what)
    _record("table/" + T.name_of(r), round(ratio, 4))
    assert ratio <= 1.0 and (sratio is None or sratio <= 1.0)


def test_small_records_include_the_kv_projections_and_a_batched_row():
    names = [T.name_of(r) for r in SMALL]
    assert sum(1 for r in SMALL if r["P"] % 77 == 0 and r["K"] == 1024 and r["ksize"] == 1) >= 3, names
    assert any(r["batch"] == 8 for r in SMALL), names


# ---------------------------------------------------------------------------------------------------------------------- stale entries
# (name, record arguments, the configuration planted under the launch's key, why the launch must not run it); shapes no other test uses
STALE = [
    ("splitk_under_per_pixel_bias", dict(n=1, C0=512, Q=96, Ho=10, Wo=12, bias_per_pixel=1), 12, "split-K with a per-pixel bias"),
    ("splitk_for_fp32_output", dict(n=1, C0=512, Q=96, Ho=10, Wo=12, out_f32=1), 14, "split-K with an fp32 output"),
    ("bk64_for_96_channels", dict(n=2, C0=96, Q=64, Ho=10, Wo=12, ksize=3, ops=("bias", "res0")), 7, "BK = 64 with C0 = 96"),
    ("halo_for_1x1", dict(n=2, C0=128, Q=64, Ho=10, Wo=12), 77, "a halo form for a 1x1"),
    ("xs_for_k256", dict(n=2, C0=256, Q=64, Ho=8, Wo=16), 25, "the X-stationary kernel with K = 256"),
]


def _planted(lib, r, cfg):
    key = (ctypes.c_int * 8)(*r["key"])
    assert lib.ladi_igemm_tune_lookup(key) == 0, "the shape of this case has an entry of its own: %s" % r["key"]
    return key


@pytest.mark.parametrize("name,args,cfg,why", STALE, ids=[s[0] for s in STALE])
def test_stale_or_colliding_entry_falls_back_and_stays_right(lib, name, args, cfg, why):
    """an entry the launch cannot run (a stale row, or a key that folds two epilogues into one bit) is re-validated: the launch falls back to
    the cost model, runs something admissible and computes the right output"""
    r = T.make_record(**args)
    pb = T.Problem(r)
    key = _planted(lib, r, cfg)
    try:
        assert lib.ladi_igemm_tune_put(key, cfg) == 0
        res = _launch(pb, lib, 0)
    finally:
        assert lib.ladi_igemm_tune_put(key, 0) in (cfg, 0)
    what = "%s (%s) %s" % (name, why, res["sel"])
    assert res["rc"] == 0, "%s: rc = %d (%s)" % (what, res["rc"], _lib.last_error())
    got, src = res["sel"]
    assert src in (3, 4) and got != cfg, what
    assert lib.ladi_igemm_cfg_admissible(ctypes.byref(res["desc"]), 1, got, 0) == 1 and lib.ladi_igemm_cfg_admissible(ctypes.byref(res["desc"]), 1, cfg, 1) == 0, what
    ratio, _ = pb.judge(res, what)
    _record("stale/" + name, dict(ratio=round(ratio, 4), cfg=got))
    assert ratio <= 1.0


def test_planted_valid_entry_is_served(lib):
    """the counterpart: a planted configuration the launch CAN run comes back as {that configuration, table}"""
    r = T.make_record(n=2, C0=96, Q=64, Ho=10, Wo=12, ksize=3, ops=("bias", "res0"))
    pb = T.Problem(r)
    key = _planted(lib, r, 5)
    assert lib.ladi_igemm_cfg_admissible(ctypes.byref(T.descriptor(r)), 1, 5, 1) == 1
    try:
        lib.ladi_igemm_tune_put(key, 5)
        res = _launch(pb, lib, 0)
    finally:
        lib.ladi_igemm_tune_put(key, 0)
    assert res["rc"] == 0 and res["sel"] == [5, 1] and res["last"][0] == 1, (res["rc"], res["sel"], res["last"])
    ratio, _ = pb.judge(res, "planted valid cfg 5")
    _record("stale/valid_entry", round(ratio, 4))


def test_gn_ss_launch_without_an_entry_takes_the_fallback_list(lib, tuner_off):
    """GroupNorm affine of the operand, no table entry, tuner off: the cost model ranks no X-stationary form, so the fixed list decides"""
    r = T.make_record(n=2, C0=320, Q=320, Ho=8, Wo=16, ops=("bias", "gn_ss"))
    assert lib.ladi_igemm_tune_lookup((ctypes.c_int * 8)(*r["key"])) == 0
    pb = T.Problem(r)
    res = _launch(pb, lib, 0)
    assert res["rc"] == 0, (res["rc"], _lib.last_error())
    assert res["sel"][1] == 4 and res["sel"][0] in (25, 26, 27, 23, 24, 93, 94, 95) and res["last"][0] == 5, (res["sel"], res["last"])
    ratio, _ = pb.judge(res, "gn_ss fallback cfg %d" % res["sel"][0])
    _record("stale/gn_ss_list", dict(ratio=round(ratio, 4), cfg=res["sel"][0]))


# ---------------------------------------------------------------------------------------------------------------------- the product
def _dump_tool():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("dump_igemm_launches", os.path.join(T.ROOT, "tools", "dump_igemm_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_product_launches_match_the_recorded_list(lib):
    """the BASELINE configs[1] capture (B = 8, 512x384, fused loop, graph on, 2 steps) again: the set of distinct launches -- geometry, key,
    configuration, source -- equals the committed lines of that run (a stale golden fails), and every one of them is served by the shipped
    table (source 1: a miss means the table no longer covers the bench run).  Table rows no capture reaches are recorded, not asserted."""
    tool = _dump_tool()
    mod = tool.tryon_modules()
    lib.ladi_igemm_launch_log(1)
    try:
        tool.run_tryon(mod, *tool.TRYON_RUNS["b8"])
    finally:
        lib.ladi_igemm_launch_log(0)
    now = {T.identity(r): r for r in T.read_log(lib)}
    gold = {T.identity(r): r for r in T.golden_records() if "b8" in r["runs"]}
    missing = [T.name_of(gold[k]) for k in gold.keys() - now.keys()]
    new = [T.name_of(now[k]) for k in now.keys() - gold.keys()]
    assert not missing and not new, "recorded launches the run no longer makes: %s; launches the list does not hold: %s" % (missing, new)
    # source 1 alone could be this process's own earlier measurement (or LADI_TUNE_CACHE): the row must be the SHIPPED table's
    off_table = [(T.name_of(r), T.SOURCES[r["src"]]) for r in now.values() if r["src"] != 1 or SHIPPED.get(tuple(r["key"])) != r["cfg"]]
    assert not off_table, "launches of the bench run the shipped table does not serve: %s" % off_table
    reached = {tuple(r["key"]) for r in T.golden_records()}
    unreached = [" ".join(str(v) for v in row) for row in T.parse_table() if tuple(row[:8]) not in reached]
    _record("unreached_rows", unreached)
    full = {T.geometry_id(r) for r in T.golden_records()}
    _record("records", dict(golden=len(T.golden_records()), reduced=len(REDUCED), geometries=len(GEOMS),
                            at_full_size=sum(1 for q in REDUCED if T.geometry_id(q) in full)))
