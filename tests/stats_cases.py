"""The cases of tests/test_gpu_stats.py as CPU data: the problems of the producer sweep, the synthetic partial rows of the consumer cases, the
judging function both files share, and a CPU stand-in for a producer with switchable mistakes.

Fused GroupNorm statistics are a hand-over: the igemm epilogue that stores an output also writes per-channel partial rows [row][Q][2] (sum,
sum of squares of the values as stored), the launcher reports how many pixels one row covers, and group_norm() (runtime_core.cpp) hands
`rps = HW / px` rows per sample to gn_norm, gn_reduce or gn_finalize (norm.hip).  The contract between the four writers and the three
readers is: exactly n HW / px rows, rows [s rps, (s + 1) rps) belong to sample s.  judge_rows() checks exactly that against
tests/util.py stats_rows_ref_bound; tests/test_cpu_stats_ref.py shows on CPU data that it accepts every summation order and rejects each
planted mistake."""
import functools

import torch
import torch.nn.functional as F

from tests import util as U


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


# ---------------------------------------------------------------------------------------------------------------------- producer sweep
# (name, ConvProblem arguments (N, c0, c1, cout, h, w), keywords): the smallest problems at which row placement can go wrong
SWEEP = [
    # 384 pixels per sample: a multiple of 32, 64, 96 and 128 (every row height but one); 1152 pixels leave a ragged last 256-pixel tile, whose
    # idle waves have no row; Q = 96 is ragged against every channel tile
    ("ragged", (3, 64, 0, 96, 16, 24), dict(act="silu", res=True, mask=True, seed=700)),
    ("halo2d", (2, 64, 0, 128, 8, 32), dict(seed=710)),                                       # the 2-D blocked halo forms
    ("stride2", (2, 64, 0, 128, 32, 48), dict(stride=2, pad=1, seed=720)),                    # 32 x 48 -> 16 x 24
    ("upsample", (2, 64, 0, 128, 8, 12), dict(ups=1, seed=730, wscale=0.05)),                 # folded upsample 8 x 12 -> 16 x 24, bias + residual
    ("1x1res", (2, 320, 0, 320, 16, 24), dict(ksize=1, pad=0, seed=740)),                     # 1x1 with residual
    ("splitk", (2, 512, 0, 192, 16, 24), dict(act="silu", rowadd=True, seed=750)),            # deep K: the split-K rows, both forms
]
SWEEP_NAMES = [s[0] for s in SWEEP]
# problems of the demotion cases
SMALL_SAMPLES = ((2, 64, 0, 96, 8, 6), dict(act="silu", seed=760))                            # 48 pixels per sample: HW % px != 0 for every px
PLAIN = ((2, 64, 0, 96, 16, 24), dict(res=False, seed=770))                                   # bias only: what batch = 3 and out_f32 accept


def sweep_problem(name):
    return next((args, kw) for n, args, kw in SWEEP if n == name)


def expected_row_px(symbol, split, two_pass, HW):
    """pixels per statistics row a launch of the kernel `symbol` (ladi_igemm_cfg_symbol_name) must report: 32 TP -- a wave's TP 32-pixel blocks
    -- for the fused epilogue and the in-launch split-K combine, 32 for the two-pass split-K reduce (always the form of the loader / consumer
    kernel's split-K, whose waves do not all reach the epilogue); 0 where a sample is not a whole number of rows (the launcher then demotes:
    no statistics) and for the X-stationary kernel, which has none"""
    if "<" not in symbol:
        return 0
    name, a = symbol.split("<")[0], [int(v) for v in symbol.split("<")[1].rstrip(">").split(",")]
    tp = a[3] if name in ("igemm_kernel", "igemm_lc_kernel") else a[1]
    px = 32 if split > 1 and (two_pass or name == "igemm_lc_kernel") else 32 * tp
    return px if HW % px == 0 else 0


# ---------------------------------------------------------------------------------------------------------------------- rows
def block_rows(x, n, HW, px):
    """the partial rows a producer with rows of px consecutive pixels writes for x [n HW, C]: float64 block sums rounded to fp32, [n HW / px][C][2]"""
    assert HW % px == 0
    v = x.double().reshape(n * HW // px, px, -1)
    return torch.stack([v.sum(1), (v * v).sum(1)], -1).float()


def rows_buffer(rows, guard, device=None, cap=None):
    """rows [R][C][2] fp32 inside a POISON32-filled allocation: `guard` poison rows in front and behind, and (cap > R) poison rows inside the
    view behind the last row -- a reader that walks past its rows adds a NaN, a writer that writes a row too many changes a poison pattern"""
    R, C = rows.shape[0], rows.shape[1]
    cap = R if cap is None else cap
    device = U.dev() if device is None else torch.device(device)
    buf = torch.full(((guard + cap + guard) * 2 * C,), U.POISON32, dtype=torch.int32, device=device).view(torch.float32)
    g = U.Guarded(buf, cap, 2 * C, 2 * C, guard, guard)
    if R:
        g.view[:R].copy_(rows.reshape(R, 2 * C).to(device))
    assert g.ptr % 16 == 0
    return g


def poisoned_rows(P, Q, guard=32, device=None):
    """the statistics buffer of a launch: room for the worst case, ceil(P / 32) rows (what the runtime reserves: runtime_core.cpp alloc_part),
    all poison, between guard rows that cover the most rows a workgroup tile can hold (512 pixels / 32)"""
    return rows_buffer(torch.zeros((0, Q, 2)), guard, device, cap=(P + 31) // 32)


def assert_all_poison(g, what):
    bits = g._bits()
    bad = bits != U.POISON32
    assert not bool(bad.any()), "%s: the statistics buffer was touched (%d words; first at row %d of the view, column %d)" % (
        what, int(bad.sum()), int(bad.nonzero()[0]) // g.ld - g.pre, int(bad.nonzero()[0]) % g.ld)


def judge_rows(g, px, stored, n, HW, what):
    """g: the statistics buffer after a launch that reported rows of px pixels (rows_buffer / poisoned_rows); stored: the output the launch
    stored, [n HW, Q] (any float dtype, fp16 values).  Exactly n HW / px rows are written, every channel of them finite; everything else is
    still poison; per sample and channel the rows add up (in float64) to the statistics of the stored output within stats_rows_ref_bound.
    Returns the worst err / bound."""
    Q = g.C // 2
    assert px > 0 and HW % px == 0, (what, px, HW)
    rps = HW // px
    R = n * rps
    assert R <= g.rows, (what, R, g.rows)
    bits = g._bits().reshape(g.pre + g.rows + g.post, g.ld)[g.pre:g.pre + g.rows]
    poison = bits == U.POISON32
    if bool(poison[:R].any()):
        r, c = (int(v) for v in poison[:R].nonzero()[0])
        raise AssertionError("%s: %d of the %d x %d words of the %d rows (px = %d) were never written; first at row %d (sample %d, row %d of its %d), "
                             "channel %d (octet %d of %d)" % (what, int(poison[:R].sum()), R, 2 * Q, R, px, r, r // rps, r % rps, rps, c // 2, c // 16, (Q + 7) // 8))
    if not bool(poison[R:].all()):
        r, c = (int(v) for v in (~poison[R:]).nonzero()[0])
        raise AssertionError("%s: %d words behind the last of the %d rows (px = %d) were written; first at row %d, channel %d"
                             % (what, int((~poison[R:]).sum()), R, px, R + r, c // 2))
    U.assert_untouched(g, what + " statistics buffer")
    rows = g.cpu()[:R].double().reshape(n, rps, Q, 2)
    if not bool(torch.isfinite(rows).all()):
        s, r, c, k = (int(v) for v in (~torch.isfinite(rows)).nonzero()[0])
        raise AssertionError("%s: non-finite statistics; first at sample %d, row %d of %d, channel %d (%s)" % (what, s, r, rps, c, ("sum", "sumsq")[k]))
    got = rows.sum(1)                                             # [n, Q, 2]
    ssum, ssq, bsum, bsq = U.stats_rows_ref_bound(stored, n, HW)
    worst = 0.0
    for k, (ref, bound, name) in enumerate(((ssum, bsum, "sum"), (ssq, bsq, "sum of squares"))):
        err = (got[..., k] - ref).abs()
        tiny = 2.0 ** -126                                        # a channel the mask zeroed everywhere: the bound is 0 and so is the error
        ratio = err / bound.clamp_min(tiny)
        bad = err > bound
        if bool(bad.any()):
            i = int(torch.where(bad, ratio, torch.zeros(())).reshape(-1).argmax())
            s, c = divmod(i, Q)
            raise AssertionError("%s: the %s of %d of %d (sample, channel) pairs is outside the bound (rows of %d pixels, %d per sample); worst at sample %d, "
                                 "channel %d (octet %d): rows add up to %.9g, stored output %.9g, err %.3g, bound %.3g"
                                 % (what, name, int(bad.sum()), bad.numel(), px, rps, s, c, c // 8, float(got[s, c, k]), float(ref[s, c]), float(err[s, c]), float(bound[s, c])))
        worst = max(worst, float(ratio.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------- a CPU producer
class EmulatedProducer:
    """N = 2, 64 -> 96 at 16 x 24, SiLU + residual + mask on the CPU, with the values at every point of the epilogue where statistics could be
    taken by mistake: t (activation, rounded to fp16), t + res (before the mask), and the stored output fp16((t + res) (1 - mask))"""

    def __init__(self, seed=780):
        self.n, self.Q, self.HW, self.px = 2, 96, 384, 128
        x, w = rand((2, 64, 16, 24), seed), rand((96, 64, 3, 3), seed + 1, 1 / 24.0)
        b, res = rand((96,), seed + 2, 0.1), rand((2, 96, 16, 24), seed + 3)
        mask = (torch.rand((2, 1, 16, 24), generator=torch.Generator().manual_seed(seed + 4)) > 0.5).double()
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
        t = F.silu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).half().double()
        self.before_residual = flat((t * (1.0 - mask)).half().double())
        self.before_mask = flat((t + res.double()).half().double())
        self.stored = flat(((t + res.double()) * (1.0 - mask)).half().double())

    def rows(self, defect=None):
        """the statistics buffer a producer leaves (CPU): faithful, or with one planted defect"""
        src = dict(before_residual=self.before_residual, before_mask=self.before_mask).get(defect, self.stored)
        rows = block_rows(src, self.n, self.HW, self.px)
        if defect == "row_in_other_sample":            # the last row of sample 0 and the first of sample 1 change places
            rps = self.HW // self.px
            rows[[rps - 1, rps]] = rows[[rps, rps - 1]]
        g = rows_buffer(rows, 4, device="cpu", cap=(self.n * self.HW + 31) // 32)
        if defect == "last_octet_poison":              # the ragged channel tile's last 8 channels are never written
            g.view[:rows.shape[0], 2 * (self.Q - 8):] = torch.tensor([U.POISON32], dtype=torch.int32).view(torch.float32)
        if defect == "phantom_row":                    # the idle wave of a ragged last pixel tile writes a row of zeros behind the last one
            g.view[rows.shape[0]] = 0.0
        return g


DEFECTS = ("row_in_other_sample", "last_octet_poison", "before_residual", "before_mask", "phantom_row")


@functools.lru_cache(maxsize=None)
def emulated_producer():
    return EmulatedProducer()


# ---------------------------------------------------------------------------------------------------------------------- consumers
GROUPS, EPS = 32, 1e-5
# one source, C = 64: (HW, px) -> rps 1, 3, 4, 12 (what producers give at 384 pixels per sample), 96 (the one-pass kernel's limit), 97 (the first
# above it, and no multiple of the fold's 16 rows), 510 (VAE-sized)
ONE_SOURCE = [(384, 384), (384, 128), (384, 96), (384, 32), (3072, 32), (3104, 32), (16320, 32)]
# two sources 320 + 160 (group size 15 straddles the source boundary): (HW, px0, px1); px = 0: the source has no producer rows
TWO_SOURCES = [(384, 128, 32), (384, 96, 0), (64, 0, 32)]


class ConsumerCase:
    """GroupNorm over (c0 | c1) channels of n = 2 samples of HW pixels, with the float64 reference and bound for every (silu, add) the tests run"""

    def __init__(self, c0, c1, HW, seed=800):
        self.n, self.c0, self.c1, self.HW = 2, c0, c1, HW
        C = c0 + c1
        x = rand((2, C, HW, 1), seed, 2.0) + 0.5
        x = x.half().float()
        self.gamma, self.beta = (rand((C,), seed + 1, 0.1) + 1).half().float(), rand((C,), seed + 2, 0.1)
        self.add = rand((2, C, HW, 1), seed + 3)
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(2 * HW, -1)
        self.x = flat(x)
        self.refs = {}
        for silu, with_add in ((0, False), (1, True)):
            ref, bound = U.group_norm_ref_bound(x, GROUPS, self.gamma, self.beta, EPS, silu=bool(silu), add=self.add if with_add else None)
            self.refs[(silu, with_add)] = (flat(ref), flat(bound))
        self.add = flat(self.add)

    def source(self, i):
        return self.x[:, :self.c0] if i == 0 else self.x[:, self.c0:]

    def rows(self, i, px):
        return block_rows(self.source(i), self.n, self.HW, px)


@functools.lru_cache(maxsize=None)
def consumer_case(c0, c1, HW):
    return ConsumerCase(c0, c1, HW, seed=800 + HW % 97)
