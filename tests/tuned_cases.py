"""The tile selections the product runs, as test cases: shared by tests/test_cpu_tuned.py and tests/test_gpu_tuned.py.

Every convolution and projection of the product goes through ladi_launch_igemm with cfg = 0: the launcher builds a tune key, looks it up in
ladi_vton_amd/tune_gfx950.txt, re-validates the hit and falls back to the cost model.  tests/golden/igemm_product_launches.txt is the list
of distinct launch forms the product makes (tools/dump_igemm_launches.py, from the launch log of include/ladi_native.h).  This module
  * parses the shipped table and decodes its `flags` field -- the decoder is written from the comment in csrc/igemm.hip and the CPU test
    checks it against ladi_igemm_tune_key, the function the launch itself calls;
  * parses the launch-log lines into records;
  * reduce(record): the smallest problem that still runs the recorded launch's code path (fewer samples, lower image; everything else kept);
  * problem(reduced): CPU operands, float64 reference and per-element bound (tests/util.py), device operands between poison rows."""
import ctypes
import functools
import math
import os

import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "ladi_vton_amd", "tune_gfx950.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_product_launches.txt")

KEY_FIELDS = ("P", "Q", "K", "C0", "C1", "Wo", "flags", "batch")
SOURCES = {0: "explicit", 1: "table", 2: "measured", 3: "cost model", 4: "gn_ss list"}
# the bits of a launch-log line's `ops` mask (include/ladi_native.h)
OPS = ("src1", "bias", "rowadd", "rowadd_idx", "res0", "res1", "mask", "stats", "ln_gamma", "ln_scratch", "gn_ss", "bias_mul", "out_scale")
ACT_NAME = {v: k for k, v in U.ACT.items()}


# ---------------------------------------------------------------------------------------------------------------------- the shipped table
def parse_table(path=TABLE):
    """rows of tune_gfx950.txt as lists of nine integers (key, cfg); comment lines skipped; a malformed line raises"""
    rows = []
    for ln in open(path):
        if ln.startswith("#") or not ln.strip():
            continue
        v = [int(t) for t in ln.split()]
        assert len(v) == 9, ln
        rows.append(v)
    return rows


# flags, from the comment above igemm_tune_key in csrc/igemm.hip:
#   bit 0 GEGLU | bit 1 a residual | bit 2 folded upsample | bit 3 fused statistics | bits 4..5 stride | bit 6 "other epilogue" (rowadd, mask,
#   per-pixel bias, fp32 output, out_scale != 1, an activation that is not GEGLU) | bit 7 LayerNorm of the operand | bits 8..10 ksize |
#   bit 12 GroupNorm affine of the operand | bit 13 bias_mul not in {0, 1}
FLAG_BITS = dict(geglu=(0, 1), res=(1, 1), ups=(2, 1), stats=(3, 1), stride=(4, 3), other=(6, 1), ln=(7, 1), ksize=(8, 7), gn=(12, 1), bias_mul=(13, 1))


def decode_flags(flags):
    """the fields of a tune key's flags; `rest` = the bits no field owns (0 for every key the launcher can build)"""
    out, known = {}, 0
    for name, (shift, mask) in FLAG_BITS.items():
        out[name] = (flags >> shift) & mask
        known |= mask << shift
    out["rest"] = flags & ~known
    return out


def encode_flags(**f):
    return sum((int(f.get(name, 0)) & mask) << shift for name, (shift, mask) in FLAG_BITS.items())


# ---------------------------------------------------------------------------------------------------------------------- launch-log records
def parse_line(line):
    """one launch-log line ("name=value ..." as ladi_igemm_launch_log_read writes it, with or without the repeat count) -> record: a dict of
    ints, `key` and `last` lists of ints, `ops` the set of operand names present"""
    r = {}
    for tok in line.split():
        name, val = tok.split("=", 1)
        r[name] = [int(v) for v in val.split(",")] if name in ("key", "last") else int(val)
    r["opmask"] = r["ops"]
    r["ops"] = frozenset(n for i, n in enumerate(OPS) if r["opmask"] >> i & 1)
    assert len(r["key"]) == 8 and len(r["last"]) == 4, line
    return r


def read_log(lib):
    """the library's launch log as records (with their repeat counts under "n")"""
    n = lib.ladi_igemm_launch_log_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.ladi_igemm_launch_log_read(buf, n + 1)
    return [parse_line(ln) for ln in buf.value.decode().splitlines() if ln]


@functools.lru_cache(maxsize=None)
def golden_records(path=GOLDEN):
    """the records of the committed launch list, in file order, each with the runs it appeared in under "runs".  The list is shared: callers
    copy a record before they change it (reduce() and the tests do)"""
    out = []
    for ln in open(path):
        if ln.startswith("#") or not ln.strip():
            continue
        tags, line = ln.rstrip("\n").split("\t")
        r = parse_line(line)
        r["runs"] = tuple(tags.split(","))
        out.append(r)
    return out


def python_key(r):
    """the tune key of a record, from the decoder's side: the record's geometry and operands through encode_flags"""
    geglu = r["act"] == U.ACT["geglu"]
    other = bool(r["ops"] & {"rowadd", "mask", "out_scale"}) or r["bias_per_pixel"] or r["out_f32"] or (r["act"] != U.ACT["none"] and not geglu)
    flags = encode_flags(geglu=geglu, res=bool(r["ops"] & {"res0", "res1"}), ups=r["ups"], stats="stats" in r["ops"], stride=r["stride"], other=other,
                         ln="ln_gamma" in r["ops"], ksize=r["ksize"], gn="gn_ss" in r["ops"], bias_mul="bias_mul" in r["ops"])
    return [r["P"], r["Q"], r["K"], r["C0"], r["C1"], r["Wo"], flags, r["batch"]]


GEOMETRY = ("C0", "C1", "ld0", "ld1", "Hs", "Ws", "Ho", "Wo", "P", "ksize", "stride", "pad", "ups", "Q", "K", "ldw", "bias_per_pixel", "rowadd_stride", "act",
            "ldr0", "ldr1", "ldo", "out_f32", "gn_hw", "bs_src0", "bs_w", "bs_out", "bs_res", "batch", "opmask")


def identity(r):
    """what test_product_launches_match_the_recorded_list compares: geometry, key, cfg and source"""
    return tuple(r[f] for f in GEOMETRY) + tuple(r["key"]) + (r["cfg"], r["src"])


_DUMMY = 1 << 20          # an aligned non-null address for descriptors nothing dereferences


def descriptor(r, addr=None):
    """the ladi_igemm_desc of a record; addr: {operand name: address} for a launch, default dummy aligned non-null addresses for the operands
    the record's mask names (host-only entry points look at null / non-null only)"""
    a = (lambda n: addr[n]) if addr is not None else (lambda n: _DUMMY)
    d = _lib.IGemmDesc()
    for f in ("C0", "C1", "ld0", "ld1", "Hs", "Ws", "Ho", "Wo", "P", "ksize", "stride", "pad", "ups", "Q", "K", "ldw", "bs_src0", "bs_w", "bs_out", "bs_res",
              "bias_per_pixel", "rowadd_stride", "act", "ldr0", "ldr1", "ldo", "out_f32", "gn_hw"):
        setattr(d, f, r[f])
    d.src0, d.W, d.out = a("src0"), a("W"), a("out")
    for name, field in (("src1", "src1"), ("bias", "bias"), ("rowadd", "rowadd"), ("rowadd_idx", "rowadd_idx"), ("res0", "res0"), ("res1", "res1"),
                        ("mask", "mask"), ("stats", "stats"), ("ln_gamma", "ln_gamma"), ("ln_scratch", "ln_scratch"), ("gn_ss", "gn_ss")):
        if name in r["ops"]:
            setattr(d, field, a(name))
    if "ln_gamma" in r["ops"]:
        d.ln_beta, d.ln_eps = a("ln_beta") if addr is not None else _DUMMY, 1e-5
    d.bias_mul = r.get("bias_mul_value", 0.125) if "bias_mul" in r["ops"] else 0.0
    d.out_scale = r.get("out_scale_value", 0.5) if "out_scale" in r["ops"] else 1.0
    return d


def tune_key(lib, r):
    """(rc, key) of ladi_igemm_tune_key on the record's descriptor"""
    key = (ctypes.c_int * 8)()
    rc = lib.ladi_igemm_tune_key(ctypes.byref(descriptor(r)), r["batch"], key)
    return rc, list(key)


# ---------------------------------------------------------------------------------------------------------------------- what a launch will do
FAMILY = {1: "ring", 2: "igemm8", 3: "igemm_lc", 4: "halo", 5: "linear_xs"}
SYMBOL_FAMILY = {"igemm_kernel": 1, "igemm8_kernel": 2, "igemm_lc_kernel": 3, "igemm_halo_kernel": 4, "linear_xs_kernel": 5}


@functools.lru_cache(maxsize=None)
def cfg_tile(cfg):
    """family, channel tile bq, pixel tile bp, tp (32-pixel blocks per wave) and, for the halo forms, g2d / ups / th of configuration cfg,
    read off the template arguments of the kernel symbol the LIBRARY names for it (as tests/test_gpu_views.py _cfg_tile does)"""
    sym = _lib.load().ladi_igemm_cfg_symbol_name(cfg).decode()
    name = sym.split("<")[0]
    t = dict(family=SYMBOL_FAMILY[name], bq=0, bp=0, tp=0, g2d=0, ups=0, th=0)
    if t["family"] == 5:
        # the X-stationary kernel's symbol carries no tile: a workgroup's pixel panel is 128 pb pixels (linear_xs.hip: grid.x = P / (128 pb)) and
        # the admission rule accepts P only in whole panels, so the rule itself tells pb: the smallest multiple of 128 pixels it accepts for a
        # plain K = 320 projection (every X-stationary configuration takes that form)
        lib = _lib.load()
        for pb in (1, 2, 4):
            d = _lib.IGemmDesc()
            d.src0 = d.W = d.out = _DUMMY
            d.C0 = d.ld0 = d.K = d.Q = d.ldo = 320
            d.Hs = d.Ho = d.P = 128 * pb
            d.Ws = d.Wo = d.ksize = d.stride = 1
            d.out_scale = 1.0
            if lib.ladi_igemm_cfg_admissible(ctypes.byref(d), 1, cfg, 0):
                t.update(bp=128 * pb, tp=pb)
                break
        assert t["bp"], "no panel size found for X-stationary configuration %d" % cfg
    if "<" in sym:
        a = [int(v) for v in sym.split("<")[1].rstrip(">").split(",")]
        if name in ("igemm_kernel", "igemm_lc_kernel"):
            t.update(bq=32 * a[0] * a[2], bp=32 * a[1] * a[3], tp=a[3])
        elif name == "igemm8_kernel":
            t.update(bq=64 * a[0], bp=128 * a[1], tp=a[1])
        else:
            t.update(bq=64 * a[0], bp=32 * a[4] * a[1], tp=a[1], g2d=a[7], ups=a[8], th=a[4] * a[1])
    return t


def samples(r):
    """(samples, pixels per sample) of a record: P = n Ho Wo for the convolutions and token-wise projections; a launch whose P is no
    multiple of Ho Wo (or a batched one: `batch` problems of P pixels) is one sample of P pixels"""
    hw = r["Ho"] * r["Wo"]
    if r["batch"] == 1 and hw > 0 and r["P"] % hw == 0:
        return r["P"] // hw, hw
    return 1, r["P"]


def predict(r, cfg=None, split=None):
    """(tile_map kind, G of kind 3, stats_row_px) the launch of record r with configuration cfg reports -- a restatement of the launchers' grid
    rules (igemm_kernel.h launch_cfg, igemm8.hip, igemm_lc.hip, igemm_halo_kernel.h launch_halo) that reduce() uses to FIND a smaller problem;
    tests/test_gpu_tuned.py asserts the conditions on what the launch itself reports, never on this."""
    cfg = r["cfg"] if cfg is None else cfg
    split = r["last"][2] if split is None else split
    t = cfg_tile(cfg)
    if t["family"] == 5:
        return 0, 0, 0
    np_, nq = -(-r["P"] // t["bp"]), -(-r["Q"] // t["bq"])
    kind, G = 0, 0
    if t["family"] in (3, 4) or r["batch"] == 1 or split > 1:
        kind = 1 if np_ >= 16 else 2 if nq >= 16 else 0
    if t["family"] == 4 and not t["g2d"] and (r["batch"] == 1 or split > 1) and 13 <= np_ <= 32:
        wbytes, xbytes = r["Q"] * r["K"] * 2, (r["P"] // 4 if t["ups"] else r["P"]) * (r["C0"] + r["C1"]) * 2
        g = (np_ + 1) // 2
        if wbytes >= 3 * xbytes and nq * split * -(-np_ // g) >= 8:
            kind, G = 3, g
    px = 0
    if "stats" in r["ops"] and r["act"] != U.ACT["geglu"] and r["batch"] == 1 and not r["out_f32"]:
        px = 32 * (1 if (split > 1 and t["family"] == 3) else t["tp"])
        px = px if (r["Ho"] * r["Wo"]) % px == 0 else 0
    return kind, G, px


# ---------------------------------------------------------------------------------------------------------------------- reduce
KEPT = ("Q", "K", "C0", "C1", "Wo", "Ws", "ksize", "stride", "pad", "ups", "act", "batch", "opmask", "bias_per_pixel", "out_f32", "cfg", "ldw", "rowadd_stride")
# 2 P Q K batch of the float64 reference.  conv_ref_bound makes two such passes (the sum and |w| (*) |x|); torch's float64 convolution
# sustains about 1e11 flop/s on 8 threads, so 2.4e11 is about 5 s there and about 3 s on 16: "a few seconds"
REF_FLOP_LIMIT = 2.4e11
# record name -> reason: records that satisfy neither the conditions nor that time at any smaller size and would be judged on a pixel subset
# (the whole first and last pixel tile of the first and last sample plus 2048 seeded random pixels).  Empty: every record of the committed
# list reduces below the limit (tests/test_cpu_tuned.py asserts it), so there is no subset judge; the first entry brings it.  At most 10 %.
FULL_SIZE_ONLY = {}


def name_of(r):
    """<key>-cfg<id>; reduced_records() adds -v2, -v3 where records that differ in something the key does not hold (a row stride, the source's
    size, which of two operands one key bit stands for) share that name"""
    return r.get("name") or "-".join(str(v) for v in r["key"]) + "-cfg%d" % r["cfg"]


def _with_shape(r, n, Ho):
    """record r at n samples of height Ho: P, Hs, Ho, gn_hw and the batch strides follow, everything else is kept"""
    n0, hw0 = samples(r)
    q = dict(r)
    if Ho != r["Ho"]:
        if r["ups"] and r["Ho"] == 2 * r["Hs"]:
            if Ho % 2:
                return None
            q["Hs"] = Ho // 2
        elif r["stride"] == 2:
            q["Hs"] = 2 * Ho + (r["Hs"] - 2 * r["Ho"])
        else:
            q["Hs"] = Ho + (r["Hs"] - r["Ho"])
        if q["Hs"] < 1:
            return None
        q["Ho"] = Ho
    hw = q["Ho"] * q["Wo"]
    if r["batch"] == 1 and r["P"] == n0 * hw0 and hw0 == r["Ho"] * r["Wo"]:
        q["P"] = n * hw
    elif Ho != r["Ho"] or n != n0:
        return None
    if r["gn_hw"]:
        if r["gn_hw"] != hw0:
            return None
        q["gn_hw"] = hw
    return q


def production_shape(r):
    """(samples, pixels per sample, P) of the PRODUCTION launch a record stands for: a reduced record carries them as q["prod"]"""
    return r.get("prod") or (samples(r) + (r["P"],))


def conditions(r, q, launched=None):
    """the conditions a reduced record q must keep from its production record r (r may be q itself: a reduced record keeps production's cfg,
    last, px and, under "prod", its shape).  launched: (tile_map kind, G, split, px) read back from the launch (the GPU test); default:
    predict(q).  Returns the list of violated conditions."""
    bad = []
    t = cfg_tile(r["cfg"])
    kind0, G0, split0, px0 = r["last"][1] & 15, r["last"][1] >> 4, r["last"][2], r["px"]
    if launched is None:
        k, g, px = predict(q)
        launched = (k, g, split0, px)
    kind, G, split, px = launched
    if kind != kind0 or (kind0 == 3 and (G > 1) != (G0 > 1)):
        bad.append("tile_map %d (G %d) instead of %d (G %d)" % (kind, G, kind0, G0))
    if split != split0:
        bad.append("split-K %d instead of %d" % (split, split0))
    if px != px0:
        bad.append("stats_row_px %d instead of %d" % (px, px0))
    (n0, hw0, P0), (n, hw) = production_shape(r), samples(q)
    if n0 >= 2 and n < 2:
        bad.append("one sample where production had %d" % n0)
    if t["bp"] and hw0 > t["bp"] and hw <= t["bp"]:
        bad.append("one pixel tile per sample where production had %d" % -(-hw0 // t["bp"]))
    # not in the list the reduction was given, added here: a launch of two pixels takes the same branches as one of a whole tile with every
    # lane but two masked off, and would not see a wrong row inside the tile -- one whole pixel tile wherever production had one
    if t["bp"] and q["P"] < min(P0, t["bp"]):
        bad.append("%d pixels, less than one pixel tile of %d" % (q["P"], t["bp"]))
    return bad


def _admissible(q):
    return bool(_lib.load().ladi_igemm_cfg_admissible(ctypes.byref(descriptor(q)), q["batch"], q["cfg"], 0))


def ref_flop(q):
    return 2.0 * q["P"] * q["Q"] * q["K"] * q["batch"]


@functools.lru_cache(maxsize=None)
def _reduce(frozen):
    r = dict(frozen)
    r.pop("prod", None)                # the search below works on the record's own shape (an already reduced record: nothing smaller exists)
    r["ops"] = frozenset(n for i, n in enumerate(OPS) if r["opmask"] >> i & 1)
    r["key"], r["last"] = list(r["key"]), list(r["last"])
    n0, hw0 = samples(r)
    if r["P"] != n0 * r["Ho"] * r["Wo"] or r["batch"] != 1:
        # one "sample" of P pixels (batched products, rows that are no image): only the pixel count shrinks, as a height at Wo pixels per row
        if r["P"] % max(r["Wo"], 1) or r["Wo"] < 1:
            return r
        r = dict(r, Ho=r["P"] // r["Wo"], Hs=r["P"] // r["Wo"], Ws=r["Wo"]) if r["ksize"] == 1 else r
        n0, hw0 = samples(r)
        if r["P"] != n0 * r["Ho"] * r["Wo"]:
            return r
    if conditions(r, r):             # the model does not reproduce what production reported: nothing to search with
        return r
    cands = sorted((n * h, n, h) for n in range(1, n0 + 1) for h in range(1, r["Ho"] + 1))
    for _, n, h in cands:
        if n == n0 and h == r["Ho"]:
            break
        q = _with_shape(r, n, h)
        if q is None or conditions(r, q) or not _admissible(q):
            continue
        return q
    return r


def _freeze(r):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in r.items() if k not in ("ops", "runs", "n")))


def reduce(r):
    """The smallest problem that still runs the recorded launch's code path.  Keeps Q, K, C0, C1, Wo, Ws, the lds' excess over C, ksize, stride,
    pad, ups, act, every present operand and batch; shrinks only the sample count and the image height, to the smallest P for which
    conditions() holds and the configuration still accepts the launch.  Idempotent; a record nothing smaller satisfies comes back unchanged."""
    q = dict(_reduce(_freeze(r)))
    q["runs"] = r.get("runs", ())
    q["prod"] = production_shape(r)
    # the key of the reduced problem (P changes, nothing else); cfg / src / last / px stay the PRODUCTION record's: what the launch must match
    q["key"] = [q["P"]] + list(r["key"][1:])
    return q


def reduced_records():
    """the distinct reduced records of the golden list, sorted so that records of one geometry are neighbours"""
    seen = {}
    for r in golden_records():
        if r["rc"] != 0:
            continue
        q = reduce(r)
        seen.setdefault((geometry_id(q), q["cfg"], tuple(q["last"][1:3]), q["px"]), q)
    out, count = [], {}
    for k in sorted(seen):
        q = seen[k]
        base = name_of(q)
        count[base] = count.get(base, 0) + 1
        out.append(dict(q, name=base if count[base] == 1 else "%s-v%d" % (base, count[base])))
    return out


def geometry_id(q):
    """everything problem() depends on: records that agree in it share operands, reference and bound"""
    return tuple(q[f] for f in GEOMETRY)


# ---------------------------------------------------------------------------------------------------------------------- problem
BIAS_MUL, OUT_SCALE = 0.125, 0.5         # the values a record with bias_mul / out_scale runs with (the log holds no values; the VAE's are 2^-k)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def _geglu_pack(w, b):
    """torch order (value rows, then gate rows) -> the library's packing: 32 value rows, then their 32 gate rows, per 64-row block"""
    half = w.shape[0] // 2
    j = torch.arange(half)
    dst_v = (j // 32) * 64 + j % 32
    wi, bi = torch.zeros_like(w), torch.zeros_like(b)
    wi[dst_v], wi[dst_v + 32] = w[:half], w[half:]
    bi[dst_v], bi[dst_v + 32] = b[:half], b[half:]
    return wi, bi


def _logical_input(q, x):
    """x [n, C, Hs, Ws] -> the image the taps walk over, padded so that a pad-0 convolution of stride q.stride gives Ho x Wo: the folded upsample
    stretches the source to the logical (Ho + k - 1 - 2 pad) x (Wo + ...) image like F.interpolate(mode="nearest"), the leading pad is q.pad, the
    trailing pad whatever the last output row / column still reaches (the launcher's bounds check supplies it as zeros)"""
    k, s, pad = q["ksize"], q["stride"], q["pad"]
    if q["ups"]:
        x = F.interpolate(x, size=(q["Ho"] + k - 1 - 2 * pad, q["Wo"] + k - 1 - 2 * pad), mode="nearest")
    H, W = x.shape[2], x.shape[3]
    bottom, right = (q["Ho"] - 1) * s + k - pad - H, (q["Wo"] - 1) * s + k - pad - W
    assert bottom >= 0 and right >= 0, (q["Ho"], q["Wo"], H, W)
    return F.pad(x, (pad, right, pad, bottom))


class Problem:
    """operands (CPU), float64 reference and bound [batch, P, Qout], and the guarded device placement of one reduced record's geometry"""

    def __init__(self, q):
        self.q = q
        ops, B, P, Q, K, C0, C1, k = q["ops"], q["batch"], q["P"], q["Q"], q["K"], q["C0"], q["C1"], q["ksize"]
        n, hw = samples(q)
        self.n, self.hw = n, hw
        seed = 9000 + (P * 31 + Q * 17 + K * 13 + q["opmask"] * 7 + k) % 100003
        act = ACT_NAME[q["act"]]
        self.geglu = act == "geglu"
        self.Qout = Q // 2 if self.geglu else Q
        self.f32 = bool(q["out_f32"])
        image = B == 1 and P == n * q["Ho"] * q["Wo"] and hw == q["Ho"] * q["Wo"]
        assert image or k == 1, "a launch that is no image is a 1x1"
        shape = (n, C0 + C1, q["Hs"], q["Ws"]) if image else (1, C0, P, 1)
        nx = B if q["bs_src0"] else 1
        nw = B if q["bs_w"] else 1
        lnorm = "ln_gamma" in ops
        xs = [(rand(shape, seed + 10 * b) * (2.0 if lnorm else 1.0) + (0.3 if lnorm else 0.0)).half().float() for b in range(nx)]
        ws = [rand((Q, C0 + C1, k, k), seed + 1 + 10 * b, 1 / math.sqrt(K)) for b in range(nw)]
        if B == 1 and k == 1:                         # asymmetric weights: a fragment / swizzle / channel-slice mix-up moves a large term
            idx = torch.arange(Q)
            ws[0][idx, (idx * 7 + 3) % (C0 + C1), 0, 0] += 1.0 + (idx % 5).float()
            ws[0] = ws[0].half().float()
        bias = rand((P if q["bias_per_pixel"] else Q,), seed + 2, 0.5) if "bias" in ops else None
        rowadd = rand((Q,), seed + 3) if "rowadd" in ops else None
        nres = B if q["bs_res"] else 1
        res0 = [rand((P, self.Qout), seed + 4 + 10 * b) for b in range(nres)] if "res0" in ops else None
        res1 = [rand((P, self.Qout), seed + 5 + 10 * b) for b in range(nres)] if "res1" in ops else None
        mask = (torch.rand((P,), generator=torch.Generator().manual_seed(seed + 6)) > 0.5).float() if "mask" in ops else None
        bias_mul = BIAS_MUL if "bias_mul" in ops else 1.0
        out_scale = OUT_SCALE if "out_scale" in ops else 1.0
        # ---- the operand the product multiplies: LayerNorm / GroupNorm affine of the pixel rows, rounded to fp16 (x_err: tests/test_gpu_views.py)
        self.extra = {}
        x_in, x_err = xs, [None] * nx
        if lnorm or "gn_ss" in ops:
            assert k == 1 and nx == 1 and not C1
            t = xs[0].permute(0, 2, 3, 1).reshape(P, C0).double()
            if lnorm:
                gamma, beta = (1.0 + 0.1 * rand((C0,), seed + 7)).half().float(), (0.1 * rand((C0,), seed + 8)).half().float()
                xin, lb = U.layer_norm_ref_bound(t, gamma, beta, 1e-5)
                xe = 0.5 * U.ulp16(xin.abs() + lb) + lb
                self.extra["ln"] = (gamma, beta)
            else:
                g = torch.Generator().manual_seed(seed + 9)
                scale, shift = 0.5 + torch.rand((n, C0), generator=g), torch.randn((n, C0), generator=g) * 0.3
                self.extra["gn"] = torch.stack([scale, shift], dim=-1).contiguous()
                sc, sh = (v.double().repeat_interleave(hw, 0) for v in (scale, shift))
                xin = t * sc + sh
                eb = 2 * U.U32 * ((t * sc).abs() + sh.abs())
                xe = 0.5 * U.ulp16(xin.abs() + eb) + eb
            x_in, x_err = [xin.t().reshape(1, C0, P, 1)], [xe.t().reshape(1, C0, P, 1)]
            image = False                          # a 1x1 on the normalised pixel rows: the reference runs on them as one column of P pixels
        # ---- reference and bound, element by element of the batch
        refs, bounds = [], []
        for b in range(B):
            xb, wb, eb = x_in[b % nx].double(), ws[b % nw].double(), x_err[b % nx]
            if image:
                xb = _logical_input(q, xb)
            if self.geglu:
                assert xb.shape[3] == 1 and k == 1 and not (res0 or res1 or mask is not None or rowadd is not None)
                X2 = xb.reshape(xb.shape[1], -1).t()
                ref, bound = U.geglu_ref_bound(X2, wb.reshape(Q, -1), bias if bias is not None else torch.zeros(Q),
                                               x_err=eb.reshape(eb.shape[1], -1).t() if eb is not None else None)
            else:
                if image:
                    to4 = lambda v: v.reshape(n, q["Ho"], q["Wo"], -1).permute(0, 3, 1, 2)
                    back = lambda v: v.permute(0, 2, 3, 1).reshape(P, -1)
                else:
                    to4 = lambda v: v.reshape(1, P, 1, -1).permute(0, 3, 1, 2)
                    back = lambda v: v.permute(0, 2, 3, 1).reshape(P, -1)
                bb = bias
                if bias is not None and q["bias_per_pixel"]:
                    bb = to4(bias.reshape(P, 1))
                ref, bound = U.conv_ref_bound(xb, wb, bias=bb, rowadd=rowadd, act=act, stride=q["stride"] if image else 1, padding=0,
                                              res=to4(res0[b % nres]) if res0 else None, res1=to4(res1[b % nres]) if res1 else None,
                                              mask=to4(mask.reshape(P, 1)) if mask is not None else None, x_err=eb,
                                              bias_mul=float(torch.tensor(bias_mul, dtype=torch.float32)), out_scale=float(torch.tensor(out_scale, dtype=torch.float32)),
                                              bias_per_pixel=bool(q["bias_per_pixel"]))
                ref, bound = back(ref), back(bound)
            refs.append(ref)
            bounds.append(bound)
        self.ref, self.bound = torch.stack(refs), torch.stack(bounds)
        self.cpu = dict(x=xs, w=ws, bias=bias, rowadd=rowadd, res0=res0, res1=res1, mask=mask)
        self.bias_mul, self.out_scale = bias_mul, out_scale
        self.dev = None

    # ------------------------------------------------------------------------------------------------------------------ device side
    def place(self):
        """the device operands, each a view between poison rows with the record's row stride excess (built once, launches only read them)"""
        if self.dev is not None:
            return self.dev
        q, c = self.q, self.cpu
        ops, B, P, Q, C0, C1, k = q["ops"], q["batch"], q["P"], q["Q"], q["C0"], q["C1"], q["ksize"]
        guard = max(q["Ws"], q["Wo"]) + 2
        d = {}
        rows_of = lambda x, lo, hi: x[:, lo:hi].permute(0, 2, 3, 1).reshape(-1, hi - lo).half()
        place = lambda ts, ld: (U.guarded(ts[0], ld=ld, pre_rows=guard, post_rows=guard) if len(ts) == 1 else U.guarded_batch(ts, ld=ld, pre_rows=guard, post_rows=guard))
        d["src0"] = place([rows_of(x, 0, C0) for x in c["x"]], q["ld0"])
        if "src1" in ops or C1:
            d["src1"] = place([rows_of(c["x"][0], C0, C0 + C1)], q["ld1"])
        wp = [w.permute(0, 2, 3, 1).reshape(Q, -1) for w in c["w"]]
        bias = c["bias"]
        if self.geglu:
            wp[0], bias = _geglu_pack(wp[0], bias if bias is not None else torch.zeros(Q))
        d["W"] = place([w.half() for w in wp], q["ldw"] or q["K"])
        keep = {}
        if bias is not None and "bias" in ops:
            keep["bias"] = bias.half().to(U.dev())
        if c["rowadd"] is not None:
            if "rowadd_idx" in ops:            # row 1 of a table with the record's row stride; the other rows and the padding columns are poison
                st = q["rowadd_stride"]
                tab = torch.full((2 * st + Q,), U.POISON32, dtype=torch.int32).view(torch.float32)
                tab[st:st + Q] = c["rowadd"]
                keep["rowadd"], keep["rowadd_idx"] = tab.to(U.dev()), torch.tensor([1], dtype=torch.int32, device=U.dev())
            else:
                keep["rowadd"] = c["rowadd"].float().to(U.dev())
        for name, ld in (("res0", q["ldr0"]), ("res1", q["ldr1"])):
            if c[name] is not None:
                d[name] = place([t.half() for t in c[name]], ld)
        if c["mask"] is not None:
            pad = (-P) % 8
            m = torch.cat([c["mask"], torch.zeros(pad)]).reshape(-1, 8).half()
            d["mask"] = U.guarded(m, pre_rows=2 * guard, post_rows=2 * guard)
        if "ln" in self.extra:
            keep["ln_gamma"], keep["ln_beta"] = (v.half().to(U.dev()) for v in self.extra["ln"])
        if "gn" in self.extra:
            keep["gn_ss"] = self.extra["gn"].to(U.dev())
        self.dev = dict(guarded=d, plain=keep)
        return self.dev

    def launch(self, lib, cfg):
        """one ladi_op_igemm_stats launch into fresh guarded outputs; returns dict(rc, out, stats, px, last, sel)"""
        q = self.q
        dev = self.place()
        g, plain = dev["guarded"], dev["plain"]
        B, P = q["batch"], q["P"]
        odt = torch.float32 if self.f32 else torch.float16
        if B > 1:
            out = U.guarded_batch([torch.full((P, self.Qout), float("nan"), dtype=odt) for _ in range(B)], ld=q["ldo"], pre_rows=4, post_rows=4)
        else:
            out = U.guarded_out(P, self.Qout, ld=q["ldo"], pre_rows=4, post_rows=4, dtype=odt)
        addr = {n: v.ptr for n, v in g.items()}
        addr.update({n: v.data_ptr() for n, v in plain.items()})
        addr["out"] = out.ptr
        stats = scratch = None
        if "stats" in q["ops"]:
            from tests import stats_cases as SC
            stats = SC.poisoned_rows(P, q["Q"])
            addr["stats"] = stats.ptr
        if "ln_scratch" in q["ops"]:
            scratch = U.guarded_out(P, q["C0"], pre_rows=2, post_rows=2)
            addr["ln_scratch"] = scratch.ptr
        r = dict(q)
        bs = lambda name: getattr(g.get(name), "bs", 0)
        r.update(bs_src0=bs("src0"), bs_w=bs("W"), bs_out=out.bs if B > 1 else 0, bs_res=bs("res0") or bs("res1"))
        d = descriptor(r, addr)
        d.bias_mul = float(self.bias_mul) if "bias_mul" in q["ops"] else 0.0
        d.out_scale = float(self.out_scale)
        px = ctypes.c_int(0)
        rc = lib.ladi_op_igemm_stats(ctypes.byref(d), B, cfg, ctypes.byref(px), _lib.stream_ptr())
        torch.cuda.synchronize()
        last, sel = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
        lib.ladi_igemm_last_launch(last)
        lib.ladi_igemm_last_selection(sel)
        return dict(rc=rc, out=out, stats=stats, scratch=scratch, px=px.value, last=list(last), sel=list(sel), desc=d)

    def judge(self, res, what):
        """check_elem of a launch's output against the reference, untouched surroundings of the output and of every
        input, and the statistics rows where the launch reported some.  Returns (worst err / limit, worst statistics ratio or None)."""
        q = self.q
        got = res["out"].cpu().float()
        got = got.reshape(q["batch"], q["P"], self.Qout)
        t = cfg_tile(res["sel"][0]) if 1 <= res["sel"][0] else dict(bq=None, bp=None)
        loc = U.pixel_locator(self.n * q["batch"], self.hw, 1, self.Qout, t["bq"], t["bp"])
        ratio = U.check_elem(got, self.ref, self.bound, what, loc, out_f32=self.f32)
        U.assert_untouched(res["out"], what + " output")
        for name, gd in self.place()["guarded"].items():
            U.assert_untouched(gd, what + " input " + name)
        sratio = None
        if res["stats"] is not None:
            from tests import stats_cases as SC
            if res["px"] > 0:
                sratio = SC.judge_rows(res["stats"], res["px"], res["out"].cpu().double(), self.n, self.hw, what)
            else:
                SC.assert_all_poison(res["stats"], what)
        return ratio, sratio


@functools.lru_cache(maxsize=2)
def _problem(frozen):
    return Problem(dict(frozen, ops=frozenset(n for i, n in enumerate(OPS) if dict(frozen)["opmask"] >> i & 1)))


def problem(q):
    """the Problem of a reduced record; records of one geometry share it (and its reference) across configurations"""
    return _problem(tuple(sorted((k, v) for k, v in q.items() if k in GEOMETRY)))


def make_record(n, C0, Q, Ho, Wo, ksize=1, ops=("bias",), act="none", **kw):
    """a hand-made record (the stale-entry cases of tests/test_gpu_tuned.py): n samples of Ho x Wo, stride 1, dense rows plus 8 elements"""
    K = ksize * ksize * C0
    r = dict(C0=C0, C1=0, ld0=C0 + 8, ld1=0, Hs=Ho, Ws=Wo, Ho=Ho, Wo=Wo, P=n * Ho * Wo, ksize=ksize, stride=1, pad=ksize // 2, ups=0, Q=Q, K=K, ldw=0,
             bias_per_pixel=0, rowadd_stride=0, act=U.ACT[act], ldr0=Q + 8 if "res0" in ops else 0, ldr1=0, ldo=Q + 8, out_f32=0, stats_groups=0, gn_hw=0,
             bs_src0=0, bs_w=0, bs_out=0, bs_res=0, batch=1, cfg=0, src=0, rc=0, last=[0, 0, 1, 0], px=0)
    r.update(kw)
    r["opmask"] = sum(1 << OPS.index(o) for o in ops)
    r["ops"] = frozenset(ops)
    if "gn_ss" in ops:
        r["gn_hw"] = Ho * Wo
    rc, r["key"] = tune_key(_lib.load(), r)
    assert rc == 0, rc
    return r
