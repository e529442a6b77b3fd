"""The fused loop's per-evaluation plan on the host, no GPU: ladi_tryon_plan_forms (the plan_evals that TryOn::run calls) against
pipeline.feature_cache_plan and the rules of include/ladi_native.h.  A form has bit 0 cond-only, bit 1 shallow, bit 2 PAG."""
import ctypes
import itertools

import pytest

from ladi_vton_amd import _lib
from ladi_vton_amd.pipeline import feature_cache_plan

PAG_WITH_FEATURE_CACHE = -12


def plan(lib, evals, guidance=7.5, table=None, phi=0.0, pag=None, flags=None, first_step=0, steps=None):
    """-> the list of forms, or (rc, message) of a refusal"""
    def arr(ctype, v):
        return ((ctype * len(v))(*v), len(v)) if v is not None else (None, 0)
    out = (ctypes.c_ubyte * max(evals, 1))()
    rc = lib.ladi_tryon_plan_forms(evals, first_step, evals if steps is None else steps, guidance, *arr(ctypes.c_float, table), phi,
                                   *arr(ctypes.c_float, pag), *arr(ctypes.c_ubyte, flags), out)
    return list(out[:evals]) if rc == evals else (rc, _lib.last_error())


def test_cache_promotion_and_cond_only_sweep(lib):
    """every evals in 1 .. 6, every feature-cache pattern whose flag 0 is 1, every guidance table over {1.0, 7.5}: bit 1 is
    feature_cache_plan's promoted plan, bit 0 the table's <= 1 entries -- of a CFG-shaped run: a table without an entry > 1 (all 1.0) is a
    run without CFG, whose evaluations all run over the B conditional samples as form bit 0 = 0, like a scalar guidance of 1.0"""
    n = 0
    for evals in range(1, 7):
        for tail in itertools.product((0, 1), repeat=evals - 1):
            flags = (1,) + tail
            for table in itertools.product((1.0, 7.5), repeat=evals):
                cfg = any(g > 1.0 for g in table)
                cond_only = [cfg and g <= 1.0 for g in table]
                forms = plan(lib, evals, table=table, flags=flags)
                whole = feature_cache_plan(evals, flags, cond_only)
                assert [bool(f & 1) for f in forms] == cond_only, (flags, table, forms)
                assert [bool(f & 2) for f in forms] == [not w for w in whole], (flags, table, forms)
                assert not any(f & 4 for f in forms)
                n += 1
    assert n == sum(2 ** (e - 1) * 2 ** e for e in range(1, 7))


@pytest.mark.parametrize("guidance", [0.0, 1.0, 1.5, 7.5])
def test_scalar_guidance_without_rescale_is_never_cond_only(lib, guidance):
    """today's `guided` rule: without a schedule and with phi == 0 the scales are no table, and no evaluation is cond-only"""
    for evals in (1, 4):
        assert plan(lib, evals, guidance=guidance) == [0] * evals
        assert plan(lib, evals, guidance=guidance, flags=[1] + [0] * (evals - 1)) == [0] + [2] * (evals - 1)
    # with phi > 0 the scalar becomes a table: a scale > 1 gives no cond-only evaluation either, a scale <= 1 is a run without CFG
    assert plan(lib, 4, guidance=guidance, phi=0.5) == [0] * 4


def test_pag_table_sets_bit_2_where_positive(lib):
    pag = [3.0, 0.0, 0.5, 0.0, 0.0, 1e-3]
    assert plan(lib, 6, pag=pag) == [4, 0, 4, 0, 0, 4]
    # with a guidance cut-off: the cond-only evaluations keep their PAG bit
    assert plan(lib, 6, table=[7.5, 7.5, 7.5, 1.0, 1.0, 1.0], pag=pag) == [4, 0, 4, 1, 1, 5]
    # without CFG
    assert plan(lib, 6, guidance=1.0, pag=pag) == [4, 0, 4, 0, 0, 4]


def test_pag_table_of_zeros_is_no_table(lib):
    for kw in (dict(), dict(table=[7.5, 1.0, 7.5, 1.0]), dict(flags=[1, 0, 0, 1]), dict(table=[1.0, 7.5, 7.5, 1.0], flags=[1, 0, 0, 0], phi=0.7)):
        assert plan(lib, 4, pag=[0.0] * 4, **kw) == plan(lib, 4, **kw)


def test_refusals_keep_codes_and_messages(lib):
    rc, msg = plan(lib, 4, table=[7.5] * 3)
    assert rc == -9 and msg == "tryon: the guidance schedule has 3 entries, this run has 4 evaluations (PNDM: steps + 1)"
    rc, msg = plan(lib, 4, pag=[3.0] * 3)
    assert rc == -9 and "PAG table has 3 entries, this run has 4 evaluations" in msg
    rc, msg = plan(lib, 4, flags=[1, 0, 1, 0, 1])
    assert rc == -10 and msg == "tryon: the feature-cache plan has 5 entries, this run has 4 evaluations (PNDM: steps + 1)"
    # a run that starts at a later step says so
    rc, msg = plan(lib, 4, flags=[1, 0], first_step=6, steps=10)
    assert rc == -10 and msg.endswith("this run has 4 evaluations (PNDM: steps + 1; the run starts at step 6 of 10)")
    rc, msg = plan(lib, 4, flags=[0, 1, 1, 1])
    assert rc == -10 and "feature-cache plan must start with a whole evaluation" in msg
    rc, msg = plan(lib, 4, pag=[0.0, 0.0, 2.0, 0.0], flags=[1, 0, 1, 0])
    assert rc == PAG_WITH_FEATURE_CACHE and "feature-cache plan is not supported" in msg
    # the order of the run's checks: guidance schedule, PAG table, PAG with a cache, the cache plan
    assert plan(lib, 4, table=[7.5] * 3, pag=[3.0] * 3, flags=[0])[0] == -9
    assert plan(lib, 4, pag=[3.0] * 4, flags=[0])[0] == PAG_WITH_FEATURE_CACHE
    # bad arguments of the entry itself
    assert plan(lib, 0)[0] == -1
    assert lib.ladi_tryon_plan_forms(4, 0, 4, 7.5, None, 0, 0.0, None, 0, None, 0, None) == -1
