"""Operands beyond 32-bit byte offsets, as test cases: shared by tests/test_cpu_far.py (host only) and tests/test_gpu_far.py.

The product sends tensors of several gigabytes through its kernels (a batch-32 run at 512 x 384 decodes [B H W, 256] fp16 = 3.2 GB in one
launch), while every operator test runs on a few megabytes.  The far regime is reached here with tiny problems: every entry point takes row
strides and per-sample / batch strides, so a 3 x 3 convolution over four samples of 8 x 8 pixels at a row stride of 2^24 + 8 halves places
sample 1 at the 2 GiB mark and sample 2 at 4 GiB while it touches 64 columns of each row.  Compute and the float64 reference stay as small as
in tests/test_gpu_views.py; only the allocation (tests/util.py guarded_far: poison everywhere outside the operand) is large.

This module holds
  * the mirror of the library's span guard (include/ladi_native.h, rc -20), written from the header's formula, and of the halo / X-stationary
    byte limits, for the host-only boundary tests;
  * FarConv: one convolution / linear problem (CPU operands, float64 reference and bound) that can be placed with any stride per operand;
  * the stride choosers (ld_for_bytes) the cases share."""
import ctypes
import math

import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from tests import tuned_cases as T
from tests import util as U

LIMIT = 0x7FFFFFFF            # num_records of the kernels' buffer descriptors: what a 32-bit byte offset may reach
MARK31, MARK32 = 1 << 31, 1 << 32
DUMMY = 1 << 20               # an aligned non-null address for descriptors nothing dereferences
FAMILY = T.FAMILY

# one small and one large (8-wave where the family has one) tile per tiled family: (cfg, pixel tile)
#   ring   9 <2,2,2,1> BK64: 128 x 64      19 <2,4,2,2> BK32, 8 waves: 128 x 256      20 <4,2,2,2> BK32, 8 waves: 256 x 128
#   igemm8 56 <2,1>: 128 x 128             33 <4,2>: 256 x 256
#   lc     66: 128 x 64    62: 128 x 128   65: 128 x 256
TILED = dict(ring=(9, 20, 19), igemm8=(56, 33), igemm_lc=(66, 62, 65))
HALO, HALO_UPS, XS, XS_RES = (77, 84), (106,), (23, 25), (25,)
SPLIT_K = 11                  # cfg 9 + split-K 2 (ring, 64-pixel tiles)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def ld_for_bytes(rows, nbytes, esize=2):
    """the smallest row stride (elements, a multiple of 8) at which row `rows` - 1 of an operand starts at or behind byte `nbytes`"""
    return (-(-nbytes // (esize * max(rows - 1, 1))) + 7) // 8 * 8 + 8


# ---------------------------------------------------------------------------------------------------------------------- mirrors of the rules
def tile_span(d, bp):
    """(span of the pixel operands, span of the weight, ns) of a launch with descriptor d on tiles of bp pixels (0: a tile inside one sample),
    from the formula in include/ladi_native.h (ladi_igemm_desc, rc -20)"""
    HoWo, HsWs = d.Ho * d.Wo, d.Hs * d.Ws
    ns = 0
    if bp:
        samples = -(-d.P // HoWo)
        ns = max(0, min((HoWo - math.gcd(bp, HoWo) + bp - 1) // HoWo, samples - 1))
    back_px = 0 if d.ups else d.pad * d.Ws + d.pad
    last = ns * HsWs + HsWs - 1 + back_px
    span = 2 * (last * d.ld0 + d.C0)
    if d.C1:
        span = max(span, 2 * (last * d.ld1 + d.C1))
    return span, 2 * ((d.Q - 1) * (d.ldw or d.K) + d.K), ns


def halo_bytes(d, ups_form=False):
    """what igemm_halo.hip compares with 0x7FFFFFFF: P max(ld0, ld1) 2 (P ld0 2 for the folded-upsample forms)"""
    return d.P * (d.ld0 if ups_form else max(d.ld0, d.ld1)) * 2


def admissible(lib, d, cfg, batch=1, strict=0):
    return bool(lib.ladi_igemm_cfg_admissible(ctypes.byref(d), batch, cfg, strict))


def tune_key_rc(lib, d, batch=1):
    key = (ctypes.c_int * 8)()
    return lib.ladi_igemm_tune_key(ctypes.byref(d), batch, key)


def largest_admissible(lib, d, field, cfg, lo, hi, batch=1):
    """the largest multiple of 8 in [lo, hi] for d.<field> at which configuration cfg is admissible (admissible at lo, not at hi; the rule is
    monotone in a stride): host-side bisection with ladi_igemm_cfg_admissible.  d is left at that value."""
    lo, hi = lo // 8, hi // 8
    setattr(d, field, lo * 8)
    assert admissible(lib, d, cfg, batch), (field, cfg, lo * 8)
    setattr(d, field, hi * 8)
    assert not admissible(lib, d, cfg, batch), (field, cfg, hi * 8)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        setattr(d, field, mid * 8)
        if admissible(lib, d, cfg, batch):
            lo = mid
        else:
            hi = mid
    setattr(d, field, lo * 8)
    return lo * 8


def bp_of(cfg):
    return T.cfg_tile(cfg)["bp"]


def family_of(cfg):
    return FAMILY[T.cfg_tile(cfg)["family"]]


# ---------------------------------------------------------------------------------------------------------------------- convolution problems
FORMS = dict(conv3x3=dict(), conv3x3_s2=dict(stride=2), conv1x1=dict(ksize=1, pad=0), ups=dict(ups=1), two_src=dict(c1=64))


class FarConv:
    """one convolution / linear problem of N samples: CPU operands, float64 reference and bound (tests/util.py conv_ref_bound), and the
    descriptor's geometry.  Nothing is placed on a device here: place() does that, with a row stride per operand."""

    def __init__(self, N, h, w, c0=64, c1=0, cout=64, ksize=3, stride=1, pad=1, ups=0, act="none", res=True, res1=False, mask=False, seed=900):
        cin = c0 + c1
        self.N, self.h, self.w, self.c0, self.c1, self.cout = N, h, w, c0, c1, cout
        self.ksize, self.stride, self.pad, self.ups, self.act = ksize, stride, pad, ups, act
        self.x = rand((N, cin, h, w), seed)
        self.wt = rand((cout, cin, ksize, ksize), seed + 1, 1 / math.sqrt(ksize * ksize * cin))
        self.b = rand((cout,), seed + 2, 0.1)
        xe = F.interpolate(self.x, scale_factor=2.0, mode="nearest") if ups else self.x
        s = F.conv2d(xe[:1], self.wt[:1], stride=stride, padding=pad)
        self.Ho, self.Wo = s.shape[2], s.shape[3]
        self.P = N * self.Ho * self.Wo
        self.r0 = rand((N, cout, self.Ho, self.Wo), seed + 4) if res else None
        self.r1 = rand((N, cout, self.Ho, self.Wo), seed + 6) if res1 else None
        self.m = (torch.rand((N, 1, self.Ho, self.Wo), generator=torch.Generator().manual_seed(seed + 5)) > 0.5).float() if mask else None
        ref, bound = U.conv_ref_bound(xe, self.wt, bias=self.b, act=act, res=self.r0, res1=self.r1, mask=self.m, stride=stride, padding=pad)
        self.ref = ref.permute(0, 2, 3, 1).reshape(self.P, cout)
        self.bound = bound.permute(0, 2, 3, 1).reshape(self.P, cout)
        self.K = ksize * ksize * cin

    def rows(self, name):
        """[rows, C] fp16 CPU tensor of a pixel operand (src0, src1, res0, res1), NHWC flattened"""
        t = dict(src0=self.x[:, :self.c0], src1=self.x[:, self.c0:], res0=self.r0, res1=self.r1)[name]
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).half().contiguous()

    def near_ld(self, name):
        return dict(src0=self.c0, src1=self.c1, res0=self.cout, res1=self.cout, out=self.cout)[name] + 64

    def packed_weight(self):
        """[cout, taps (c0 + c1)] fp16: tap-major, inside a tap source 0's channels, then source 1's (all multiples of 64 here)"""
        return self.wt.permute(0, 2, 3, 1).reshape(self.cout, self.K).half().contiguous()

    def desc(self, ld=None, addr=None):
        """the launch's descriptor; ld: {operand: row stride} (default: the near stride C + 64), addr: {operand: address} (default: dummy
        non-null addresses for the operands the problem has -- the host-only entry points look at null / non-null only)"""
        ld, a = dict(ld or {}), (lambda n: addr[n]) if addr is not None else (lambda n: DUMMY)
        L = lambda n: ld.get(n, self.near_ld(n))
        d = _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = a("src0"), self.c0, L("src0")
        if self.c1:
            d.src1, d.C1, d.ld1 = a("src1"), self.c1, L("src1")
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = self.h, self.w, self.Ho, self.Wo, self.P
        d.ksize, d.stride, d.pad, d.ups = self.ksize, self.stride, self.pad, self.ups
        d.W, d.Q, d.K, d.ldw = a("W"), self.cout, self.K, 0
        d.bias, d.act, d.out_scale = a("bias"), U.ACT[self.act], 1.0
        if self.r0 is not None:
            d.res0, d.ldr0 = a("res0"), L("res0")
        if self.r1 is not None:
            d.res1, d.ldr1 = a("res1"), L("res1")
        if self.m is not None:
            d.mask = a("mask")
        d.out, d.ldo = a("out"), L("out")
        return d

    def place(self, ld=None):
        return PlacedConv(self, ld or {})


class PlacedConv:
    """a FarConv's inputs on the device, each pixel operand a guarded_far view at its row stride (ld[name], default near); launches read them
    only, so every configuration of a case shares them.  close() drops the allocations (the caller's `finally`)."""

    def __init__(self, pb, ld):
        self.pb, self.ld = pb, dict(ld)
        self.g = {}
        for name in ("src0", "src1", "res0", "res1"):
            if (name == "src1" and not pb.c1) or (name == "res0" and pb.r0 is None) or (name == "res1" and pb.r1 is None):
                continue
            self.g[name] = U.guarded_far(pb.rows(name), self.ld.get(name, pb.near_ld(name)))
        self.W = pb.packed_weight().to(U.dev())
        self.B = pb.b.half().to(U.dev())
        self.M = U.guarded_far(pb.m.permute(0, 2, 3, 1).reshape(-1, 8).half(), 8) if pb.m is not None else None

    def close(self):
        self.g.clear()
        self.W = self.B = self.M = None

    def largest_offset(self):
        """the largest byte offset (from its base) of any operand element of this placement, and of the output at its stride"""
        ldo = self.ld.get("out", self.pb.near_ld("out"))
        return max([g.last_byte for g in self.g.values()] + [((self.pb.P - 1) * ldo + self.pb.cout) * 2 - 1])

    def launch(self, lib, cfg, stats=None):
        """one launch into a fresh far-guarded output; (rc, output, px reported for the statistics rows or None)"""
        pb = self.pb
        ldo = self.ld.get("out", pb.near_ld("out"))
        out = U.guarded_far_out(pb.P, pb.cout, ldo)
        addr = dict(src0=self.g["src0"].ptr, W=self.W.data_ptr(), bias=self.B.data_ptr(), out=out.ptr)
        for name in ("src1", "res0", "res1"):
            if name in self.g:
                addr[name] = self.g[name].ptr
        if self.M is not None:
            addr["mask"] = self.M.ptr
        d = pb.desc(dict(self.ld, out=ldo), addr)
        if stats is None:
            rc, px = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, _lib.stream_ptr()), None
        else:
            d.stats = stats.ptr
            pxc = ctypes.c_int(-1)
            rc, px = lib.ladi_op_igemm_stats(ctypes.byref(d), 1, cfg, ctypes.byref(pxc), _lib.stream_ptr()), None
            px = pxc.value
        torch.cuda.synchronize()
        return rc, out, px

    def check(self, out, what):
        """per-element check of a launch's output and the poison of the output and of every input; the worst err / limit"""
        pb = self.pb
        ratio = U.check_elem(out.cpu().float(), pb.ref, pb.bound, what, U.pixel_locator(pb.N, pb.Ho, pb.Wo, pb.cout))
        U.assert_untouched_far(out, what + " output")
        self.check_inputs(what)
        return ratio

    def check_inputs(self, what):
        for name, g in list(self.g.items()) + [("mask", self.M)]:
            if g is not None:
                U.assert_untouched_far(g, what + " input " + name)


def assert_nothing_written(out, what):
    """a refused launch launched nothing: the output operand still holds the NaN it was created with and its surroundings the poison"""
    assert bool(torch.isnan(out.cpu()).all()), what + ": a refused launch wrote output elements"
    U.assert_untouched_far(out, what + " output of the refused launch")


def last_launch(lib):
    info = (ctypes.c_int * 4)()
    assert lib.ladi_igemm_last_launch(info) == 0
    return dict(family=FAMILY.get(info[0], info[0]), tile_map=info[1] & 15, split=info[2], blocks=info[3])


def last_selection(lib):
    sel = (ctypes.c_int * 2)()
    assert lib.ladi_igemm_last_selection(sel) == 0
    return sel[0], sel[1]
