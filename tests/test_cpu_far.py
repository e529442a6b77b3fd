"""The byte limits of the implicit-GEMM launch, host only: ladi_igemm_tune_key and ladi_igemm_cfg_admissible dereference nothing, so they
can be asked about launches of any size.

  * the halo forms and the X-stationary kernel stop being admissible exactly at the byte count their sources state, rule by rule;
  * the span guard of the tiled kernels (include/ladi_native.h, rc -20) flips exactly where its formula says -- tests/far_cases.py tile_span
    is written from the header --, for every tiled family, tile size and form, aligned and straddling;
  * the guard refuses nothing the product launches: every record of tests/golden/igemm_product_launches.txt at B = 32, 512 x 384 and at
    B = 8, 1024 x 768 (the largest sizes of BASELINE.md) has an admissible configuration and an accepted tune key."""
import ctypes
import math

import pytest

from ladi_vton_amd import _lib
from tests import far_cases as FC
from tests import tuned_cases as T

LIMIT = FC.LIMIT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _bisect(lib, d, field, cfg, batch=1):
    return FC.largest_admissible(lib, d, field, cfg, (getattr(d, field) + 7) // 8 * 8, 1 << 30, batch)


# ---------------------------------------------------------------------------------------------------------------------- halo, linear_xs
@pytest.mark.parametrize("cfg,kind,geom,field", [
    (77, "ring-halo", dict(N=4, h=8, w=8), "ld0"), (84, "ring-halo", dict(N=3, h=16, w=24), "ld0"),
    (77, "ring-halo", dict(N=4, h=8, w=8, c1=64), "ld1"), (77, "ring-halo", dict(N=4, h=8, w=8, c1=64), "ld0"),
    (103, "2-D blocked", dict(N=2, h=8, w=32), "ld0"), (100, "2-D blocked", dict(N=2, h=8, w=32, c1=64), "ld1"),
    (106, "folded upsample", dict(N=3, h=8, w=8, ups=1), "ld0"), (104, "folded upsample", dict(N=2, h=8, w=12, ups=1), "ld0")])
def test_halo_admission_flips_at_its_byte_limit(lib, cfg, kind, geom, field):
    """igemm_halo.hip: P max(ld0, ld1) 2 < 0x7FFFFFFF for the ring-halo and 2-D blocked forms, P ld0 2 for the folded-upsample forms (P the
    OUTPUT pixels).  The largest admissible stride satisfies the rule, the next multiple of 8 breaks it."""
    pb = FC.FarConv(**geom)
    d = pb.desc()
    ld = _bisect(lib, d, field, cfg)
    ups = kind == "folded upsample"
    assert FC.halo_bytes(d, ups) < LIMIT, (kind, ld, FC.halo_bytes(d, ups))
    setattr(d, field, ld + 8)
    assert FC.halo_bytes(d, ups) >= LIMIT and not FC.admissible(lib, d, cfg), (kind, ld)
    assert FC.tune_key_rc(lib, d) == 0          # another family still runs it: the launch as such is not refused


@pytest.mark.parametrize("cfg,P", [(25, 128), (26, 384), (27, 128)])
def test_linear_xs_admission_flips_at_its_residual_byte_limit(lib, cfg, P):
    """linear_xs.hip: P ldr0 2 < 0x7FFFFFFF for the residual form.  (Its second rule, Q K 2 < 0x7FFFFFFF for the weight, cannot flip: the
    kernel's LDS budget, (Q / qs) 2 bytes of bias among it, refuses such a Q long before -- nothing to test.)  The pixel operand itself has
    no limit there: the kernel addresses it with 64 bits."""
    pb = FC.FarConv(N=1, h=P, w=1, c0=320, cout=320, ksize=1, pad=0)
    d = pb.desc()
    ld = _bisect(lib, d, "ldr0", cfg)
    assert P * ld * 2 < LIMIT <= P * (ld + 8) * 2, (ld, P)
    d.ldr0, d.ld0 = pb.near_ld("res0"), (1 << 30) - 8
    assert FC.admissible(lib, d, cfg) and FC.tune_key_rc(lib, d) == 0


# ---------------------------------------------------------------------------------------------------------------------- the span guard
ALL_TILED = [c for cfgs in FC.TILED.values() for c in cfgs] + [FC.SPLIT_K]
GEOMS = [("aligned", dict(N=4, h=16, w=16)), ("straddling", dict(N=3, h=8, w=8)), ("ragged", dict(N=3, h=10, w=6))]


@pytest.mark.parametrize("geom_name,geom", GEOMS)
@pytest.mark.parametrize("form", sorted(FC.FORMS))
def test_span_guard_flips_where_its_formula_says(lib, form, geom_name, geom):
    """for every tiled configuration of tests/far_cases.py that takes the form at ordinary strides: the largest admissible ld0 (and ld1 of the
    two-source form) has span < 0x7FFFFFFF and the next multiple of 8 reaches it, span computed by far_cases.tile_span from the header's
    formula with the configuration's pixel tile.  aligned: 256-pixel samples, every tile inside one (ns = 0); straddling: 64-pixel samples,
    tiles of 128 / 256 pixels span 2 / 3 of them; ragged: 60-pixel samples, gcd(bp, 60) = 4."""
    pb = FC.FarConv(**geom, **FC.FORMS[form])
    seen = 0
    for cfg in ALL_TILED:
        for field in ("ld0", "ld1") if pb.c1 else ("ld0",):
            d = pb.desc()
            if not FC.admissible(lib, d, cfg):
                continue                                      # the family does not take this form at any stride (loader / consumer: no upsample)
            seen += 1
            bp = FC.bp_of(cfg)
            ld = _bisect(lib, d, field, cfg)
            span, _, ns = FC.tile_span(d, bp)
            assert span < LIMIT, (form, geom_name, cfg, field, ld, span)
            setattr(d, field, ld + 8)
            span2, _, _ = FC.tile_span(d, bp)
            assert span2 >= LIMIT, (form, geom_name, cfg, field, ld, span2)
            HoWo = pb.Ho * pb.Wo
            assert ns == (0 if HoWo % bp == 0 else min((HoWo - math.gcd(bp, HoWo) + bp - 1) // HoWo, pb.N - 1))
            # the argument-level refusal: only when even a tile inside one sample is out of reach
            one = FC.tile_span(d, 0)[0]
            assert FC.tune_key_rc(lib, d) == (-20 if one >= LIMIT else 0), (form, geom_name, cfg, field, one)
    assert seen >= 6, (form, geom_name, seen)


def test_span_guard_single_sample_refusal_is_an_argument_refusal(lib):
    """tune_key returns -20 exactly from the stride at which a tile inside ONE sample reaches the limit, for every form -- and never for a
    shape the X-stationary kernel takes, whose pixel operand has no limit"""
    for form, kw in sorted(FC.FORMS.items()):
        pb = FC.FarConv(N=3, h=8, w=8, **kw)
        d = pb.desc()
        lo, hi = 8, (1 << 30) // 8
        while hi - lo > 1:
            mid = (lo + hi) // 2
            d.ld0 = mid * 8
            lo, hi = (mid, hi) if FC.tune_key_rc(lib, d) == 0 else (lo, mid)
        d.ld0 = lo * 8
        assert FC.tile_span(d, 0)[0] < LIMIT and FC.tune_key_rc(lib, d) == 0, form
        d.ld0 = lo * 8 + 8
        assert FC.tile_span(d, 0)[0] >= LIMIT and FC.tune_key_rc(lib, d) == -20, form
        assert not any(FC.admissible(lib, d, c) for c in range(1, lib.ladi_igemm_cfg_count() + 1)), form
    xs = FC.FarConv(N=1, h=128, w=1, c0=320, cout=320, ksize=1, pad=0, res=False)
    d = xs.desc()
    d.ld0 = (1 << 30) - 8
    assert FC.tile_span(d, 0)[0] >= LIMIT and FC.tune_key_rc(lib, d) == 0
    assert FC.admissible(lib, d, 25) and not FC.admissible(lib, d, 9)


def test_span_guard_covers_the_weight(lib):
    """the weight descriptor has the same 32-bit reach from W: 2 ((Q - 1) ldw + K) < 0x7FFFFFFF, for the tiled and the halo families"""
    pb = FC.FarConv(N=4, h=8, w=8, cout=128)
    for cfg in (9, 56, 66, 77):
        d = pb.desc()
        d.ldw = pb.K
        ldw = _bisect(lib, d, "ldw", cfg)
        assert FC.tile_span(d, 0)[1] < LIMIT <= 2 * ((pb.cout - 1) * (ldw + 8) + pb.K), (cfg, ldw)
    d.ldw = ldw + 8
    assert FC.tune_key_rc(lib, d) == -20


def test_span_guard_of_a_batched_launch_counts_one_element(lib):
    """batch > 1: the batch stride is added to the descriptor's base with 64 bits, so only one element's rows count -- bs_src0 may be anything"""
    pb = FC.FarConv(N=1, h=256, w=1, ksize=1, pad=0, res=False)
    d = pb.desc()
    d.bs_src0 = d.bs_out = (1 << 33) + 64
    for cfg in (9, 20, 56):
        assert FC.admissible(lib, d, cfg, batch=3), cfg
        ld = _bisect(lib, d, "ld0", cfg, batch=3)
        assert FC.tile_span(d, FC.bp_of(cfg))[0] < LIMIT, (cfg, ld)
        d.ld0 = ld + 8
        assert FC.tile_span(d, FC.bp_of(cfg))[0] >= LIMIT
        d.ld0 = pb.near_ld("src0")


# ---------------------------------------------------------------------------------------------------------------------- the product
def _scaled(r, f):
    """record r of the launch list at f times its batch: a batched launch runs f times the elements, a launch over pixel rows f times the
    rows (one sample of P rows when it was recorded that way: the token-wise projections)"""
    r = dict(r)
    if f == 1:
        return r
    if r["batch"] > 1:
        r["batch"] *= f
        return r
    one = r["Ws"] == 1 and r["Hs"] == r["P"] and r["Ho"] == r["P"]
    r["P"] *= f
    if one:
        r["Hs"] = r["Ho"] = r["P"]
    if r["gn_hw"] and one:
        pass                                            # pixels per sample of the GroupNorm affine: unchanged by the batch
    return r


@pytest.mark.parametrize("run,factor", [("b32", 1), ("b8", 4), ("hr", 8)])
def test_span_guard_refuses_no_product_launch(lib, run, factor):
    """every distinct launch the product makes (tests/golden/igemm_product_launches.txt), at the largest sizes of BASELINE.md -- B = 32 at
    512 x 384 (the b32 records as captured, and the b8 records times 4) and B = 8 at 1024 x 768 (the hr records, captured at B = 1, times 8):
    the tune key is accepted and at least one configuration is admissible.  The largest single-sample span of the list is reported."""
    ncfg = lib.ladi_igemm_cfg_count()
    recs = [r for r in T.golden_records() if run in r["runs"]]
    assert len(recs) >= 100
    worst = 0
    for r in recs:
        s = _scaled(r, factor)
        d = T.descriptor(s)
        key = (ctypes.c_int * 8)()
        assert lib.ladi_igemm_tune_key(ctypes.byref(d), s["batch"], key) == 0, s
        ok = [c for c in range(1, ncfg + 1) if lib.ladi_igemm_cfg_admissible(ctypes.byref(d), s["batch"], c, 0)]
        assert ok, "no admissible configuration for %s" % s
        if factor == 1 and s["cfg"]:
            assert s["cfg"] in ok, "the configuration the product ran (%d) is no longer admissible: %s" % (s["cfg"], s)
        worst = max(worst, FC.tile_span(d, 0)[0])
    assert worst < LIMIT
    print("largest single-sample span of run %s x %d: %d bytes (%.1f %% of the limit)" % (run, factor, worst, 100.0 * worst / LIMIT))
