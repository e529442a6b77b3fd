"""The tile selection path on the CPU: the shipped table's structure, the committed list of product launches against the table and the key
function the launch itself calls (the host-only entry points of include/ladi_native.h load without a GPU), reduce(), and the judge of
tests/test_gpu_tuned.py on synthetic outputs with planted defects."""
import ctypes

import pytest
import torch

from tests import tuned_cases as T
from tests import util as U

ROWS = T.parse_table()
SHIPPED = {tuple(r[:8]): r[8] for r in ROWS}
RECORDS = T.golden_records()
MEASURED = {(tuple(r["key"]), r["cfg"]) for r in RECORDS if r["src"] == 2}
IDS = ["%d-%s" % (i, T.name_of(r)) for i, r in enumerate(RECORDS)]


# ---------------------------------------------------------------------------------------------------------------------- table structure
def test_table_rows_are_well_formed(lib):
    n = lib.ladi_igemm_cfg_count()
    assert len(ROWS) >= 270
    keys = [tuple(r[:8]) for r in ROWS]
    assert len(set(keys)) == len(keys), "duplicate key: the later row silently wins"
    for P, Q, K, C0, C1, Wo, flags, batch, cfg in ROWS:
        row = (P, Q, K, C0, C1, Wo, flags, batch, cfg)
        f = T.decode_flags(flags)
        assert 1 <= cfg <= n, row
        assert f["rest"] == 0 and f["ksize"] in (1, 3) and f["stride"] in (1, 2) and f["ups"] in (0, 1), (row, f)
        assert T.encode_flags(**f) == flags, (row, f)
        assert K == f["ksize"] ** 2 * (C0 + C1), row
        assert C0 % 32 == 0 and C1 % 32 == 0 and C0 > 0, row
        assert Wo >= 1 and P % Wo == 0, row
        assert not f["geglu"] or Q % 64 == 0, row
        assert batch in (1, 8, 32), row


def test_table_lookup_reads_every_shipped_row(lib):
    """ladi_igemm_tune_lookup loads the table as a launch does: every row comes back"""
    for row in ROWS:
        assert lib.ladi_igemm_tune_lookup((ctypes.c_int * 8)(*row[:8])) == row[8], row


def test_tune_put_is_process_local_and_reversible(lib):
    key = (ctypes.c_int * 8)(123457, 96, 96, 96, 0, 7, T.encode_flags(ksize=1, stride=1), 1)
    assert lib.ladi_igemm_tune_lookup(key) == 0
    assert lib.ladi_igemm_tune_put(key, 3) == 0 and lib.ladi_igemm_tune_lookup(key) == 3
    assert lib.ladi_igemm_tune_put(key, 5) == 3 and lib.ladi_igemm_tune_lookup(key) == 5
    assert lib.ladi_igemm_tune_put(key, lib.ladi_igemm_cfg_count() + 1) == -1 and lib.ladi_igemm_tune_lookup(key) == 5
    assert lib.ladi_igemm_tune_put(key, 0) == 5 and lib.ladi_igemm_tune_lookup(key) == 0
    assert lib.ladi_igemm_tune_put(key, 0) == 0


def test_tune_key_returns_the_launch_refusals(lib):
    """the refusals sit in front of the key: the entry point returns the launch's codes and leaves the key alone"""
    base = next(r for r in RECORDS if r["ksize"] == 3 and r["batch"] == 1 and not r["C1"] and not r["out_f32"])
    for change, rc in ((dict(ksize=2), -1), (dict(C0=base["C0"] + 8), -2), (dict(K=base["K"] + 8), -3), (dict(ld0=base["ld0"] + 4), -4), (dict(P=0), -5),
                       (dict(batch=2, C1=32, K=9 * (base["C0"] + 32)), -18), (dict(out_f32=1, act=U.ACT["silu"]), -19)):
        q = dict(base, **change)
        key = (ctypes.c_int * 8)(*([-7] * 8))
        assert lib.ladi_igemm_tune_key(ctypes.byref(T.descriptor(q)), q["batch"], key) == rc, (change, rc)
        assert list(key) == [-7] * 8, change
    g = dict(base, act=U.ACT["geglu"], Q=96, opmask=base["opmask"] & 2)
    g["ops"] = frozenset(n for i, n in enumerate(T.OPS) if g["opmask"] >> i & 1)
    assert T.tune_key(lib, g)[0] == -6


# ---------------------------------------------------------------------------------------------------------------------- golden records
def test_golden_list_is_not_empty_and_covers_the_runs():
    runs = {t for r in RECORDS for t in r["runs"]}
    assert {"b8", "b32", "hr", "text", "vision", "adapter", "refine", "tps"} <= runs, runs
    assert all(r["rc"] == 0 for r in RECORDS)


@pytest.mark.parametrize("i", range(len(RECORDS)), ids=IDS)
def test_golden_record_key_lookup_and_admission(lib, i):
    r = RECORDS[i]
    rc, key = T.tune_key(lib, r)
    assert rc == 0 and key == r["key"] == T.python_key(r), (key, r["key"], T.python_key(r))
    f = T.decode_flags(key[6])
    assert f["rest"] == 0 and f["ksize"] == r["ksize"] and f["stride"] == r["stride"] and f["ups"] == r["ups"], f
    assert r["src"] in (1, 2), "the product reached the cost model: %s" % T.SOURCES[r["src"]]
    if r["src"] == 1 and tuple(key) not in SHIPPED:
        # served from the process's own table: a run of the capture measured this shape before (recorded with source 2)
        assert (tuple(key), r["cfg"]) in MEASURED, "source 1, but neither the shipped table nor an earlier measurement holds the key"
    elif r["src"] == 1:
        assert SHIPPED[tuple(key)] == r["cfg"] == lib.ladi_igemm_tune_lookup((ctypes.c_int * 8)(*key)), "the table no longer holds the recorded selection"
    else:
        assert tuple(key) not in SHIPPED and lib.ladi_igemm_tune_lookup((ctypes.c_int * 8)(*key)) == 0, "measured although the table holds the key"
    # a table hit and a measured choice are both judged by the strict rule, at the full production shape
    assert lib.ladi_igemm_cfg_admissible(ctypes.byref(T.descriptor(r)), r["batch"], r["cfg"], 1) == 1, "the selection is no longer admissible"
    if r["last"][2] > 1:            # split-K rows
        assert r["batch"] == 1 and r["act"] != U.ACT["geglu"] and not r["out_f32"] and not r["bias_per_pixel"], r


def test_bench_run_is_served_by_the_table():
    """every launch of the BASELINE configs[1] capture (the bench run) has source 1: the shipped table covers it"""
    miss = [T.name_of(r) for r in RECORDS if "b8" in r["runs"] and (r["src"] != 1 or SHIPPED.get(tuple(r["key"])) != r["cfg"])]
    assert not miss, miss


# ---------------------------------------------------------------------------------------------------------------------- reduce
@pytest.mark.parametrize("i", range(len(RECORDS)), ids=IDS)
def test_reduce_keeps_what_it_must(lib, i):
    r = RECORDS[i]
    q = T.reduce(r)
    for f in T.KEPT:
        assert q[f] == r[f], (f, q[f], r[f])
    for ld, c in (("ld0", "C0"), ("ld1", "C1")):
        assert q[ld] - q[c] == r[ld] - r[c], ld
    qout = lambda v: v["Q"] // 2 if v["act"] == U.ACT["geglu"] else v["Q"]
    assert q["ldo"] - qout(q) == r["ldo"] - qout(r) and q["ldr0"] == r["ldr0"] and q["ldr1"] == r["ldr1"]
    assert q["P"] <= r["P"] and q["key"][1:] == r["key"][1:] and q["key"][0] == q["P"]
    assert not T.conditions(r, q) or (q["P"] == r["P"]), T.conditions(r, q)
    again = T.reduce(q)
    assert T.geometry_id(again) == T.geometry_id(q), "reduce is not idempotent"
    rc, key = T.tune_key(lib, q)
    assert rc == 0 and key == q["key"], (rc, key, q["key"])
    assert lib.ladi_igemm_cfg_admissible(ctypes.byref(T.descriptor(q)), q["batch"], q["cfg"], 0) == 1


def test_full_size_only_list_is_short_and_names_real_records():
    red = T.reduced_records()
    names = {T.name_of(q) for q in red}
    assert set(T.FULL_SIZE_ONLY) <= names, set(T.FULL_SIZE_ONLY) - names
    assert len(T.FULL_SIZE_ONLY) <= 0.10 * len(red), (len(T.FULL_SIZE_ONLY), len(red))
    slow = [T.name_of(q) for q in red if T.ref_flop(q) > T.REF_FLOP_LIMIT and T.name_of(q) not in T.FULL_SIZE_ONLY]
    assert not slow, "reduced records whose float64 reference is over the time limit and that are not listed: %s" % slow
    # records that do not shrink at all stay few: predict() restates the launchers' grid rules, and a drift between the two shows up as
    # records that silently fall back to their production size (conditions(r, r) no longer holds)
    drifted = [T.name_of(r) for r in RECORDS if T.conditions(r, r)]
    assert not drifted, "predict() no longer reproduces what production reported for: %s" % drifted
    full = {T.geometry_id(r) for r in RECORDS}
    at_full = [T.name_of(q) for q in red if T.geometry_id(q) in full]
    assert len(at_full) <= 0.10 * len(red), at_full


def test_x_stationary_records_keep_their_panels():
    """the X-stationary kernel's tile is its pixel panel (128 pb pixels, asked of the admission rule): its records keep two panels per sample
    wherever production had two, like every tiled family"""
    xs = [q for q in red_xs()]
    assert xs
    for q in xs:
        bp = T.cfg_tile(q["cfg"])["bp"]
        assert bp in (128, 256), (q["cfg"], bp)
        n0, hw0, P0 = q["prod"]
        n, hw = T.samples(q)
        assert (hw > bp or hw0 <= bp) and (n >= 2 or n0 < 2) and q["P"] >= min(P0, bp), (T.name_of(q), q["prod"], n, hw, bp)


def red_xs():
    return [q for q in T.reduced_records() if q["last"][0] == 5]


# ---------------------------------------------------------------------------------------------------------------------- the judge
def _representatives():
    """two reduced records with a bias and a residual and no activation or mask: a 3x3 convolution and a 1x1 projection"""
    red = T.reduced_records()
    ok = lambda q: {"bias", "res0"} <= q["ops"] and q["act"] == U.ACT["none"] and not (q["ops"] & {"mask", "ln_gamma", "gn_ss", "out_scale", "bias_mul", "res1"}) \
        and q["batch"] == 1 and T.samples(q)[0] >= 2 and T.ref_flop(q) < 2e10 and q["Q"] >= 64
    conv = min((q for q in red if ok(q) and q["ksize"] == 3), key=T.ref_flop)
    lin = min((q for q in red if ok(q) and q["ksize"] == 1), key=T.ref_flop)
    return conv, lin


@pytest.fixture(scope="module", params=[0, 1], ids=["conv3x3", "linear"])
def synthetic(request):
    q = _representatives()[request.param]
    pb = T.Problem(q)
    return q, pb, pb.ref[0].half().float()           # what a faithful kernel stores: the reference rounded to fp16


def _judge(pb, got, what):
    return U.check_elem(got[None], pb.ref, pb.bound, what)


def test_judge_accepts_the_rounded_reference(synthetic):
    q, pb, good = synthetic
    assert _judge(pb, good, "faithful") <= 1.0


@pytest.mark.parametrize("defect", ["one_wrong_element", "row_of_the_other_sample", "swapped_32_channel_blocks", "missing_residual", "bias_twice"])
def test_judge_rejects_planted_defects(synthetic, defect):
    q, pb, good = synthetic
    n, hw = T.samples(q)
    got = good.clone()
    if defect == "one_wrong_element":              # the last element holds its neighbour pixel's value
        got[-1, -1] = good[-2, -1]
    elif defect == "row_of_the_other_sample":      # the first pixel of sample 1 holds the last pixel of sample 0
        got[hw] = good[hw - 1]
    elif defect == "swapped_32_channel_blocks":
        got[:, :32], got[:, 32:64] = good[:, 32:64], good[:, :32]
    elif defect == "missing_residual":
        got = (pb.ref[0] - pb.cpu["res0"][0].double()).half().float()
    elif defect == "bias_twice":
        got = (pb.ref[0] + pb.cpu["bias"].double()[None, :]).half().float()
    with pytest.raises(AssertionError):
        _judge(pb, got, defect)
