"""Kernels on strided, offset views with poisoned surroundings, judged element by element.

The product never hands a kernel a dense, freshly allocated tensor: attention reads q / k / v out of the fused QKV buffer and the cross K/V
cache, convolutions write into out_ld 4 / 8 buffers and into caller views, LayerNorm runs on x.ld, and every tensor sits in a bump arena
between other live tensors.  Here every operand is a view (tests/util.py guarded()) inside a NaN-filled allocation: poison rows before and
after, poison in the columns [C, ld) of every row.  A read of a neighbour that is multiplied by a zero weight or probability turns the output
NaN; a vector store that spills into the padding columns or the next row changes a poison pattern (assert_untouched); a wrong border column
or a missed bias fails the per-element bound (check_elem: |got - ref| <= ulp16(ref) + bound, float64 reference, bound derived in the
*_ref_bound helpers).  The worst err / limit of every case goes into the parity record under "views/..." keys.

The tile-map cases ask the library which map the launch they judged took (ladi_igemm_last_launch), so a threshold change cannot silently
un-test a map."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from tests import util as U

pytestmark = pytest.mark.gpu

FAMILY = {1: "ring", 2: "igemm8", 3: "igemm_lc", 4: "halo", 5: "linear_xs"}


def _cfg_tile(lib, cfg):
    """(channel tile, pixel tile) of tile configuration cfg, for the failure messages: read off the template arguments of the kernel symbol the
    LIBRARY reports for it (ladi_igemm_cfg_symbol_name), so it cannot drift from csrc/igemm.hip.  igemm_kernel / igemm_lc_kernel<WQ, WP, TQ, TP,
    ...>: 32 WQ TQ x 32 WP TP; igemm8_kernel<TQ, TP, ...>: 64 TQ x 128 TP; igemm_halo_kernel<TQ, TP, NXB, NSTW, WPN, ...>: 64 TQ x 32 WPN TP"""
    sym = lib.ladi_igemm_cfg_symbol_name(cfg).decode()
    if "<" not in sym:
        return None, None
    name, a = sym.split("<")[0], [int(v) for v in sym.split("<")[1].rstrip(">").split(",")]
    if name in ("igemm_kernel", "igemm_lc_kernel"):
        return 32 * a[0] * a[2], 32 * a[1] * a[3]
    if name == "igemm8_kernel":
        return 64 * a[0], 128 * a[1]
    if name == "igemm_halo_kernel":
        return 64 * a[0], 32 * a[4] * a[1]
    return None, None


def test_every_configuration_of_this_file_has_a_tile(lib):
    """the failure messages name the tile an element falls in: every tiled configuration this file launches must parse (_cfg_tile)"""
    for cfg in FAMILY_OF:
        bq, bp = _cfg_tile(lib, cfg)
        assert bq and bp and bq % 32 == 0 and bp % 32 == 0, (cfg, lib.ladi_igemm_cfg_symbol_name(cfg), bq, bp)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def _record(test, case, ratio):
    U.record_parity("views/%s[%s]" % (test, case), round(ratio, 4))


def _last_launch(lib):
    info = (ctypes.c_int * 4)()
    assert lib.ladi_igemm_last_launch(info) == 0
    return dict(family=FAMILY.get(info[0], info[0]), tile_map=info[1] & 15, G=info[1] >> 4, split=info[2], blocks=info[3])


# ---------------------------------------------------------------------------------------------------------------------- convolutions
class ConvProblem:
    """one convolution / linear problem: CPU operands, float64 reference + bound, and the guarded device inputs (built once per problem and
    shared by every configuration that runs it; launches only read them)"""

    def __init__(self, N, c0, c1, cout, h, w, act="none", res=True, rowadd=False, mask=False, stride=1, pad=1, ups=0, ksize=3, seed=70, wscale=None):
        cin = c0 + c1
        self.N, self.c0, self.c1, self.cout, self.h, self.w = N, c0, c1, cout, h, w
        self.act, self.stride, self.pad, self.ups, self.ksize = act, stride, pad, ups, ksize
        x = _rand((N, cin, h, w), seed)
        wt = _rand((cout, cin, ksize, ksize), seed + 1, wscale or 1 / math.sqrt(ksize * ksize * cin))
        b = _rand((cout,), seed + 2, 0.1)
        te = _rand((cout,), seed + 3) if rowadd else None
        xe = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
        padding = pad
        if stride == 2 and pad == 0:                  # the VAE's Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then a pad-0 convolution
            xe, padding = F.pad(xe, (0, 1, 0, 1)), 0
        s = F.conv2d(xe[:1, :, :, :], wt[:1], stride=stride, padding=padding)
        self.Ho, self.Wo = s.shape[2], s.shape[3]
        r = _rand((N, cout, self.Ho, self.Wo), seed + 4) if res else None
        m = (torch.rand((N, 1, self.Ho, self.Wo), generator=torch.Generator().manual_seed(seed + 5)) > 0.5).float() if mask else None
        ref, bound = U.conv_ref_bound(xe, wt, bias=b, rowadd=te, act=act, res=r, mask=m, stride=stride, padding=padding)
        self.P = N * self.Ho * self.Wo
        self.ref = ref.permute(0, 2, 3, 1).reshape(self.P, cout)
        self.bound = bound.permute(0, 2, 3, 1).reshape(self.P, cout)
        # device side: every pixel operand a view with ld = C + 64 between poison rows at least W + 1 pixels deep
        guard = max(w, self.Wo) + 2
        xs0 = U.nhwc16(x[:, :c0])
        self.X0 = U.guarded(xs0, ld=xs0.shape[3] + 64, pre_rows=guard, post_rows=guard)
        self.C0p = xs0.shape[3]
        self.X1 = None
        if c1:
            xs1 = U.nhwc16(x[:, c0:])
            self.X1, self.C1p = U.guarded(xs1, ld=xs1.shape[3] + 64, pre_rows=guard, post_rows=guard), xs1.shape[3]
        self.W = U.pack_conv_weight(wt) if not c1 else self._pack_two(wt, c0)
        self.B = b.half().to(U.dev())
        self.TE = te.float().to(U.dev()) if rowadd else None
        self.R = None
        if res:
            rs = U.nhwc16(r)
            self.R = U.guarded(rs, ld=rs.shape[3] + 64, pre_rows=guard, post_rows=guard)
        self.M = U.guarded(m.permute(0, 2, 3, 1).reshape(-1, 8).half(), pre_rows=2 * guard, post_rows=2 * guard) if mask else None

    @staticmethod
    def _pack_two(wt, c0):
        """packed weight of a two-source convolution: tap-major, inside a tap source 0's (padded) channels, then source 1's"""
        co, ci, k, _ = wt.shape
        pad64 = lambda c: (c + 63) // 64 * 64
        p0, p1 = pad64(c0), pad64(ci - c0)
        out = torch.zeros((co, k * k, p0 + p1), dtype=torch.float16)
        wp = wt.permute(0, 2, 3, 1).reshape(co, k * k, ci).half()
        out[:, :, :c0] = wp[:, :, :c0]
        out[:, :, p0:p0 + ci - c0] = wp[:, :, c0:]
        return out.reshape(co, -1).contiguous().to(U.dev())

    def try_launch(self, lib, cfg, out_ld=None):
        """one ladi_op_igemm launch into a fresh guarded output; returns (return code, output)"""
        ldo = out_ld or self.cout + 8
        out = U.guarded_out(self.P, self.cout, ld=ldo, pre_rows=4, post_rows=4)
        d = _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = self.X0.ptr, self.C0p, self.X0.ld
        if self.X1 is not None:
            d.src1, d.C1, d.ld1 = self.X1.ptr, self.C1p, self.X1.ld
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = self.h, self.w, self.Ho, self.Wo, self.P
        d.ksize, d.stride, d.pad, d.ups = self.ksize, self.stride, self.pad, self.ups
        d.W, d.Q, d.K, d.ldw = self.W.data_ptr(), self.cout, self.ksize * self.ksize * (self.C0p + (self.C1p if self.X1 is not None else 0)), 0
        d.bias, d.act, d.out_scale = self.B.data_ptr(), U.ACT[self.act], 1.0
        if self.TE is not None:
            d.rowadd = self.TE.data_ptr()
        if self.R is not None:
            d.res0, d.ldr0 = self.R.ptr, self.R.ld
        if self.M is not None:
            d.mask = self.M.ptr
        d.out, d.ldo = out.ptr, ldo
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    def launch(self, lib, cfg, out_ld=None):
        """a launch that must be accepted; returns (output, what the launcher reports about the launch)"""
        rc, out = self.try_launch(lib, cfg, out_ld)
        assert rc == 0, "cfg %d refused the launch: rc = %d (%s)" % (cfg, rc, _lib.last_error())
        return out, _last_launch(lib)

    def check(self, lib, cfg, out, what):
        """per-element check of one launch's output, untouched surroundings of the output AND of every input; returns the worst err / limit"""
        bq, bp = _cfg_tile(lib, cfg)
        ratio = U.check_elem(out.cpu().float(), self.ref, self.bound, what, U.pixel_locator(self.N, self.Ho, self.Wo, self.cout, bq, bp))
        U.assert_untouched(out, what + " output")
        for name, g in (("x", self.X0), ("x2", self.X1), ("res", self.R), ("mask", self.M)):
            if g is not None:
                U.assert_untouched(g, what + " input " + name)
        return ratio

    def judge(self, lib, test, cfg, out_ld=None, repeats=1, case=None):
        """launch, per-element check, untouched surroundings of the output AND of every input, bit-equal repeats; returns the launch info"""
        out, info = self.launch(lib, cfg, out_ld)
        what = "%s cfg %d %s" % (test, cfg, info)
        ratio = self.check(lib, cfg, out, what)
        first = out.cpu()
        for i in range(repeats):
            again, info2 = self.launch(lib, cfg, out_ld)
            assert info2 == info, (what, info2)
            assert torch.equal(again.cpu(), first), "%s: repeat %d differs" % (what, i + 1)
            U.assert_untouched(again, what + " output of repeat %d" % (i + 1))
        _record(test, case or "cfg%d" % cfg, ratio)
        return info


def _kw(**kw):
    return tuple(sorted(kw.items()))


# The problem caches of this file (this one, _xs_problem, _attn_problem, _gn_problem) keep their float64 references AND their guarded device
# buffers for the whole session, so that every configuration of a problem shares one reference.  All of them together hold well under
# 100 MB on the device (the largest: the 2600 x 300 attention case, 25 MB), which is why they are not evicted.
@functools.lru_cache(maxsize=None)
def _problem_kw(args, kw):
    return ConvProblem(*args, **dict(kw))


# one or more configurations per kernel family (lists drawn from tests/test_gpu_ops.py: test_conv3x3_eight_wave_tiles, test_conv3x3_halo_resident)
RING, IGEMM8, LC, HALO1D, HALOW24 = [3, 7, 39], [32, 56], [62, 67], [74, 77, 84], [88, 89, 97]
FAMILY_OF = {**{c: "ring" for c in RING + [5, 9, 12, 14, 16, 47]}, **{c: "igemm8" for c in IGEMM8 + [36]}, **{c: "igemm_lc" for c in LC + [66, 69]},
             **{c: "halo" for c in HALO1D + HALOW24 + [80, 86, 90, 91, 109, 100, 101, 102, 103, 104, 106, 107, 108]}}


@pytest.mark.parametrize("cfg", RING + IGEMM8 + LC + HALO1D + HALOW24)
def test_conv3x3_ragged_pixel_tiles(lib, cfg):
    """N = 3, 128 -> 320 at 20 x 13 (780 pixels: ragged pixel tiles, the image rows narrower than every tile), bias + residual, strided
    operands and output.  The first / last image rows' out-of-image taps land in poison if they are read unmasked."""
    info = _problem_kw((3, 128, 0, 320, 20, 13), _kw()).judge(lib, "conv3x3_ragged_pixel_tiles", cfg)
    assert info["family"] == FAMILY_OF[cfg], info


@pytest.mark.parametrize("cfg", [7, 32, 62, 74, 88])
def test_conv3x3_two_sources(lib, cfg):
    """the virtual concat 128 + 64 channels (two guarded sources with their own strides), SiLU + residual"""
    info = _problem_kw((2, 128, 64, 320, 20, 13), _kw(act="silu", seed=83)).judge(lib, "conv3x3_two_sources", cfg)
    assert info["family"] == FAMILY_OF[cfg], info


@pytest.mark.parametrize("cfg,split", [(14, 2), (12, 4), (36, 2), (69, 2), (80, 2), (86, 2), (90, 2), (109, 8)])
def test_conv3x3_split_k(lib, cfg, split):
    """every family's split-K representative on the few-tile / deep-K problem of test_gpu_ops.py (N = 2, 512 -> 192 at 8 x 6: SiLU, time
    embedding, residual): the in-launch combine's last-arriving slice runs the epilogue into the strided output; five bit-equal repeats"""
    info = _problem_kw((2, 512, 0, 192, 8, 6), _kw(act="silu", rowadd=True, seed=60)).judge(lib, "conv3x3_split_k", cfg, repeats=5)
    assert info["family"] == FAMILY_OF[cfg] and info["split"] == split, info


@pytest.mark.parametrize("out_ld", [4, 8])
@pytest.mark.parametrize("cfg", [3, 7, 5, 56, 66, 84, 88])
def test_conv3x3_ragged_q_output_layers(lib, cfg, out_ld):
    """N = 2, 64 -> 3 with out_ld = 4 and 8 (the UNet's and the VAE's output layers), bias + (1 - mask): the epilogue's scalar tail, which every
    family reaches with its own LDS layout and pixel stride (ring 3 / 7 / 5, igemm8 56, loader / consumer 66, halo 84 and its W <= 24 form 88).
    Column 3 (columns 3..7) of every output pixel is poison that must survive; the pixel rows of x and the mask are guarded."""
    pb = _problem_kw((2, 64, 0, 3, 16, 12), _kw(res=False, mask=True, seed=22, wscale=0.05))
    info = pb.judge(lib, "conv3x3_ragged_q_output_layers", cfg, out_ld=out_ld, case="cfg%d-ld%d" % (cfg, out_ld))
    assert info["family"] == FAMILY_OF[cfg], info


@pytest.mark.parametrize("cfg", [3, 7, 32, 62])
@pytest.mark.parametrize("h,w,pad", [(16, 12, 1), (16, 12, 0), (15, 9, 1)])
def test_conv3x3_stride2(lib, cfg, h, w, pad):
    """stride 2 with pad 1 (UNet Downsample2D; an odd side gives ceil(side / 2)) and pad 0 (VAE Downsample2D: the trailing pad is implied by the
    bounds check -- the taps past the last row / column must read nothing)"""
    _problem_kw((2, 64, 0, 128, h, w), _kw(res=False, stride=2, pad=pad, seed=7)).judge(lib, "conv3x3_stride2", cfg, case="cfg%d-%dx%d-pad%d" % (cfg, h, w, pad))


@pytest.mark.parametrize("cfg", [3, 7, 56])
def test_conv3x3_upsample_fold(lib, cfg):
    """folded nearest-2x upsample at 8 x 6 -> 16 x 12, bias + skip"""
    _problem_kw((1, 128, 0, 64, 8, 6), _kw(ups=1, seed=10, wscale=0.05)).judge(lib, "conv3x3_upsample_fold", cfg)


@pytest.mark.parametrize("cfg", [100, 101, 102, 103])
def test_conv3x3_halo_2d(lib, cfg):
    """2-D blocked halo form: N = 2, 128 -> 128 at 16 x 64, SiLU + residual + mask through the row-strided epilogue"""
    info = _problem_kw((2, 128, 0, 128, 16, 64), _kw(act="silu", mask=True, seed=170)).judge(lib, "conv3x3_halo_2d", cfg, repeats=2)
    assert info["family"] == "halo", info


@pytest.mark.parametrize("cfg,N,cin,cout,hw,split", [(104, 2, 128, 128, (8, 12), 1), (106, 3, 64, 128, (4, 8), 1),
                                                     (107, 2, 1152, 128, (8, 12), 2), (108, 2, 1280, 128, (8, 8), 2)])
def test_conv3x3_halo_upsample(lib, cfg, N, cin, cout, hw, split):
    """the halo kernel's folded-upsample forms and their split-K forms: low-resolution rows in front of the first / behind the last sample
    are poison"""
    pb = _problem_kw((N, cin, 0, cout, hw[0], hw[1]), _kw(ups=1, seed=110, wscale=0.05 if cin < 1000 else None))
    info = pb.judge(lib, "conv3x3_halo_upsample", cfg, repeats=2)
    assert info["family"] == "halo" and info["split"] == split, info


SYMBOL_FAMILY = {"igemm_kernel": "ring", "igemm8_kernel": "igemm8", "igemm_lc_kernel": "igemm_lc", "igemm_halo_kernel": "halo", "linear_xs_kernel": "linear_xs"}
# the smallest problems at which every kind of form can still go wrong, (ConvProblem arguments, keywords), all with one sample:
EVERY_CFG_PROBLEMS = [
    ((1, 64, 0, 128, 16, 24), _kw(seed=180)),                               # 3x3 on rows of 24 pixels: ring, igemm8, lc, ring-halo and its W <= 24 forms, every split-K row
    ((1, 64, 0, 128, 8, 32), _kw(seed=181)),                                # 3x3 at 8 x 32: the 2-D blocked halo forms (W % 32 == 0, H % 8 == 0)
    ((1, 64, 0, 128, 8, 12), _kw(ups=1, seed=182, wscale=0.05)),            # folded upsample 8 x 12 -> 16 x 24: 384 pixels = whole 128- and 192-pixel tiles
    ((1, 320, 0, 320, 16, 16), _kw(res=False, ksize=1, pad=0, seed=183)),   # 1x1, K = 320, P = 256 (one 64-pixels-per-wave panel), Q / 32 = 10 (1, 2 and 5 slices)
    ((1, 640, 0, 320, 8, 16), _kw(res=False, ksize=1, pad=0, seed=184)),    # 1x1, K = 640, P = 128 (one 32-pixels-per-wave panel)
]


def test_every_configuration_launches_the_kernel_it_names(lib):
    """the dispatch generated from csrc/igemm_tiles.h, end to end: EVERY tile configuration 1..ladi_igemm_cfg_count() is launched explicitly on each
    of the problems above that it accepts, judged element by element against the float64 reference there (a form launched with another form's
    grid, split-K slab or template arguments fails the bound or the poison checks), and the family its launcher reports must be the family of
    the symbol the library names for it.  No configuration may be refused by all problems."""
    n = lib.ladi_igemm_cfg_count()
    problems = [_problem_kw(args, kw) for args, kw in EVERY_CFG_PROBLEMS]
    uncovered, worst = [], 0.0
    for cfg in range(1, n + 1):
        family = SYMBOL_FAMILY[lib.ladi_igemm_cfg_symbol_name(cfg).decode().split("<")[0]]
        accepted = 0
        for i, pb in enumerate(problems):
            rc, out = pb.try_launch(lib, cfg)
            if rc != 0:
                continue
            accepted += 1
            info = _last_launch(lib)
            assert info["family"] == family, (cfg, i, info, family)
            worst = max(worst, pb.check(lib, cfg, out, "every_configuration cfg %d problem %d %s" % (cfg, i, info)))
        if not accepted:
            uncovered.append(cfg)
    assert not uncovered, "configurations no problem of this test reaches: %s" % uncovered
    _record("every_configuration", "worst", worst)


# ---------------------------------------------------------------------------------------------------------------------- linear_xs
def _geglu_pack(w, b):
    half = w.shape[0] // 2
    wi, bi = torch.zeros_like(w), torch.zeros_like(b)
    for j in range(half):
        blk, i = divmod(j, 32)
        wi[blk * 64 + i], wi[blk * 64 + 32 + i] = w[j], w[half + j]
        bi[blk * 64 + i], bi[blk * 64 + 32 + i] = b[j], b[half + j]
    return wi, bi


@functools.lru_cache(maxsize=None)
def _xs_problem(form):
    """C = 320, Q = 320 at 16 x 24 (384 pixels = three 128-pixel panels; two samples for the GroupNorm affine), one per epilogue form"""
    C, Q, h, w = 320, 320, 16, 24
    N = 2 if form == "gn" else 1
    x = _rand((N, C, h, w), 80) * (2.0 if form == "ln" else 1.0) + (0.3 if form == "ln" else 0.0)
    x = x.half().float()
    wt = _rand((Q, C), 81, 1 / math.sqrt(C))
    for q in range(Q):
        wt[q, (q * 7 + 3) % C] += 1.0 + (q % 5)          # asymmetric: catches a fragment / swizzle / channel-slice mix-up
    wt = wt.half().float()
    b = _rand((Q,), 82, 0.1)
    P = N * h * w
    t = x.permute(0, 2, 3, 1).reshape(P, C).double()
    extra, x_err, xin = {}, None, t
    if form == "ln":
        gamma, beta = (1.0 + 0.1 * _rand((C,), 111)).half().float(), (0.1 * _rand((C,), 112)).half().float()
        xin, lb = U.layer_norm_ref_bound(t, gamma, beta, 1e-5)
        x_err = 0.5 * U.ulp16(xin.abs() + lb) + lb          # the normalised operand is rounded to fp16 before the product
        extra["ln"] = (gamma.half().to(U.dev()), beta.half().to(U.dev()))
    if form == "gn":
        g = torch.Generator().manual_seed(303)
        scale, shift = 0.5 + torch.rand((N, C), generator=g), torch.randn((N, C), generator=g) * 0.3
        extra["gn"] = torch.stack([scale, shift], dim=-1).contiguous().to(U.dev())
        sc, sh = (v.double().repeat_interleave(h * w, 0) for v in (scale, shift))
        xin = t * sc + sh
        eb = 2 * U.U32 * ((t * sc).abs() + sh.abs())        # x * scale + shift in fp32, rounded to fp16 like gn_apply_kernel
        x_err = 0.5 * U.ulp16(xin.abs() + eb) + eb
    res = None
    if form == "geglu":
        ref, bound = U.geglu_ref_bound(xin, wt, b)
        wdev, bdev = (v.half().contiguous().to(U.dev()) for v in _geglu_pack(wt, b))
    else:
        res = _rand((P, Q), 93) if form == "res" else None
        x4 = xin.t().reshape(1, C, P, 1)
        ref, bound = U.conv_ref_bound(x4, wt.reshape(Q, C, 1, 1), bias=b, padding=0,
                                      res=res.t().reshape(1, Q, P, 1) if res is not None else None,
                                      x_err=x_err.t().reshape(1, C, P, 1) if x_err is not None else None)
        ref, bound = (v.reshape(Q, P).t().contiguous() for v in (ref, bound))
        wdev, bdev = wt.half().contiguous().to(U.dev()), b.half().to(U.dev())
    X = U.guarded(x.permute(0, 2, 3, 1).half(), ld=C + 64, pre_rows=w + 2, post_rows=w + 2)
    R = U.guarded(res.half(), ld=Q + 64, pre_rows=w + 2, post_rows=w + 2) if res is not None else None
    return dict(N=N, C=C, Q=Q, h=h, w=w, P=P, X=X, W=wdev, B=bdev, R=R, ref=ref, bound=bound, extra=extra)


@pytest.mark.parametrize("form,cfg", [("plain", 25), ("plain", 93), ("res", 25), ("geglu", 25), ("geglu", 93), ("ln", 25), ("ln", 93), ("gn", 25)])
def test_linear_xs_forms(lib, form, cfg):
    """the X-stationary linear kernel, once per epilogue / prologue form (plain, residual by LDS-DMA, GEGLU, fused LayerNorm, fused GroupNorm
    affine) and ring depth: the pixel panel is read from a view with ld = C + 64, the residual from ld = Q + 64, the output written at
    ldo = Q + 8"""
    pb = _xs_problem(form)
    Qout = pb["Q"] // 2 if form == "geglu" else pb["Q"]

    def launch():
        out = U.guarded_out(pb["P"], Qout, ld=Qout + 8, pre_rows=4, post_rows=4)
        d = _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = pb["X"].ptr, pb["C"], pb["X"].ld
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = pb["h"], pb["w"], pb["h"], pb["w"], pb["P"]
        d.ksize, d.stride, d.pad, d.ups = 1, 1, 0, 0
        d.W, d.Q, d.K, d.ldw = pb["W"].data_ptr(), pb["Q"], pb["C"], 0
        d.bias, d.act, d.out_scale = pb["B"].data_ptr(), U.ACT["geglu" if form == "geglu" else "none"], 1.0
        if pb["R"] is not None:
            d.res0, d.ldr0 = pb["R"].ptr, pb["R"].ld
        if form == "ln":
            d.ln_gamma, d.ln_beta, d.ln_eps = pb["extra"]["ln"][0].data_ptr(), pb["extra"]["ln"][1].data_ptr(), 1e-5
        if form == "gn":
            d.gn_ss, d.gn_hw = pb["extra"]["gn"].data_ptr(), pb["h"] * pb["w"]
        d.out, d.ldo = out.ptr, Qout + 8
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
        assert rc == 0, "cfg %d refused the %s form: rc = %d (%s)" % (cfg, form, rc, _lib.last_error())
        torch.cuda.synchronize()
        return out, _last_launch(lib)

    out, info = launch()
    assert info["family"] == "linear_xs", info
    what = "linear_xs %s cfg %d" % (form, cfg)
    ratio = U.check_elem(out.cpu().float(), pb["ref"], pb["bound"], what, U.pixel_locator(pb["N"], pb["h"], pb["w"], Qout, 32, 128))
    U.assert_untouched(out, what + " output")
    U.assert_untouched(pb["X"], what + " input x")
    if pb["R"] is not None:
        U.assert_untouched(pb["R"], what + " input res")
    again, _ = launch()
    assert torch.equal(again.cpu(), out.cpu()), what + ": repeat differs"
    _record("linear_xs_forms", "%s-cfg%d" % (form, cfg), ratio)


# ---------------------------------------------------------------------------------------------------------------------- tile maps
@pytest.mark.parametrize("cfg,split", [(88, 1), (90, 2), (91, 4), (109, 8)])
@pytest.mark.parametrize("N,h,w", [(7, 16, 15), (13, 16, 8)])
def test_tile_map3_weight_slice_major(lib, cfg, split, N, h, w):
    """the halo kernels' weight-slice-major map in the launcher's DEFAULT mode, on the W <= 24 forms with 128 x 128 tiles and their split-K
    forms: 128 -> 640, N = 7 at 16 x 15 (P = 1680: 14 pixel tiles, the last ragged, G = 7) and N = 13 at 16 x 8 (P = 1664: 13 tiles, G = 7, the
    second group one tile short).  Weights >= 3x the pixel operand and >= 8 units in both.  The launch itself reports the map."""
    info = _problem_kw((N, 128, 0, 640, h, w), _kw(seed=130)).judge(lib, "tile_map3", cfg, repeats=10, case="cfg%d-n%d-%dx%d" % (cfg, N, h, w))
    assert info["family"] == "halo" and info["tile_map"] == 3 and info["G"] == 7 and info["split"] == split, info


@pytest.mark.parametrize("N,h,w", [(7, 24, 15), (13, 16, 12)])
def test_tile_map3_weight_slice_major_192_pixel_tiles(lib, N, h, w):
    """cfg 89 is the W <= 24 form with 128 x 192 tiles: the two shapes above give it 9 pixel tiles, under the launcher's 13-tile threshold
    for map 3, so it gets shapes of its own with the same properties -- 128 -> 896, N = 7 at 24 x 15 (P = 2520: 14 tiles of 192, the last
    ragged, G = 7) and N = 13 at 16 x 12 (P = 2496: 13 tiles, G = 7, the second group one short); weights 2.06 MB >= 3 x 0.65 MB, 14 units"""
    info = _problem_kw((N, 128, 0, 896, h, w), _kw(seed=140)).judge(lib, "tile_map3", 89, repeats=10, case="cfg89-n%d-%dx%d" % (N, h, w))
    assert info["family"] == "halo" and info["tile_map"] == 3 and info["G"] == 7 and info["split"] == 1, info


@pytest.mark.parametrize("cfg", [7, 47, 56, 62, 77, 84])
def test_tile_map1_pixel_tiles_over_xcds(lib, cfg):
    """map 1 (pixel tiles split over the 8 XCDs) with a tile count >= 16 that is not a multiple of 8: 128 -> 128, N = 5 at 32 x 14 (P = 2240:
    18 tiles of 128, the last ragged, so XCDs 0 and 1 own three tiles, the others two and an idle slot), once per family that has the map"""
    info = _problem_kw((5, 128, 0, 128, 32, 14), _kw(seed=150)).judge(lib, "tile_map1", cfg, repeats=10)
    assert info["family"] == FAMILY_OF[cfg] and info["tile_map"] == 1 and info["blocks"] == 24, info


@pytest.mark.parametrize("cfg", [5, 16])
def test_tile_map2_channel_tiles_over_xcds(lib, cfg):
    """map 2 (channel tiles split over the XCDs) with 19 channel tiles of 64 (Q = 1216, the 64 x 64 ring forms) on N = 1 at 8 x 6"""
    info = _problem_kw((1, 128, 0, 1216, 8, 6), _kw(seed=160)).judge(lib, "tile_map2", cfg, repeats=10)
    assert info["family"] == "ring" and info["tile_map"] == 2 and info["blocks"] == 24, info


# ---------------------------------------------------------------------------------------------------------------------- attention
KV_GUARD = 130      # poison rows behind the last key row: more than one whole key stage (128), so a ragged tile's over-read lands in poison


def _heads(t, n, heads, hd):
    return t.view(n, -1, heads, hd).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _attn_problem(n, heads, hd, Nq, Nk, fused, causal=False, seed=40, small=False):
    """fused: q / k / v are column slices of ONE [n T, 3C] buffer (self-attention); else q is a view with ld = C + 64 and k / v are the halves
    of a [n Nk, 2C] buffer (the cross-attention K/V cache).  small: logits of a few tenths and a positive V (see
    test_attention_small_logits_resolve_a_few_ulps)"""
    C = heads * hd
    q, k, v = _rand((n, Nq, C), seed), _rand((n, Nk, C), seed + 1), _rand((n, Nk, C), seed + 2)
    if small:
        q, k, v = (q * 0.1).half().float(), (k * 0.1).half().float(), (v.abs() + 0.5).half().float()
    else:
        k[0, Nk - 1, :hd] = q[0, 3, :hd] * 4.0       # a late spike: the rescale branch of the online softmax
    scale = hd ** -0.5
    ref, bound = U.attention_ref_bound(_heads(q, n, heads, hd), _heads(k, n, heads, hd), _heads(v, n, heads, hd), scale, causal=causal)
    flat = lambda t: t.transpose(1, 2).reshape(n * Nq, C)
    if fused:
        assert Nq == Nk
        buf = U.guarded(torch.cat([q, k, v], -1).half(), pre_rows=KV_GUARD, post_rows=KV_GUARD)
        ops = dict(q=(buf.col(0), 3 * C), k=(buf.col(C), 3 * C), v=(buf.col(2 * C), 3 * C), bufs=[buf])
    else:
        qb = U.guarded(q.half(), ld=C + 64, pre_rows=KV_GUARD, post_rows=KV_GUARD)
        kv = U.guarded(torch.cat([k, v], -1).half(), pre_rows=KV_GUARD, post_rows=KV_GUARD)
        ops = dict(q=(qb.ptr, C + 64), k=(kv.col(0), 2 * C), v=(kv.col(C), 2 * C), bufs=[qb, kv])
    return dict(ref=flat(ref), bound=flat(bound), scale=scale, C=C, **ops)


def _attn_judge(lib, test, case, pb, n, heads, hd, Nq, Nk, call):
    C = pb["C"]
    ldo = C + 8

    def launch():
        out = U.guarded_out(n * Nq, C, ld=ldo, pre_rows=4, post_rows=4)
        (q, ldq), (k, ldk), (v, ldv) = pb["q"], pb["k"], pb["v"]
        rc = call(q, k, v, out.ptr, ldq, ldk, ldv, ldo, Nq * ldq, Nk * ldk, Nk * ldv, Nq * ldo)
        assert rc == 0, (test, case, rc)
        torch.cuda.synchronize()
        return out
    out = launch()
    what = "%s %s" % (test, case)

    def loc(i):
        r, c = divmod(i, C)
        return "(sample, query, head, d) = (%d, %d, %d, %d); query tile of 128: %d, last key tile of 64 starts at key %d" % (
            r // Nq, r % Nq, c // hd, c % hd, (r % Nq) // 128, (Nk - 1) // 64 * 64)
    ratio = U.check_elem(out.cpu().float(), pb["ref"], pb["bound"], what, loc)
    U.assert_untouched(out, what + " output")
    for g in pb["bufs"]:
        U.assert_untouched(g, what + " input")
    assert torch.equal(launch().cpu(), out.cpu()), what + ": repeat differs"
    _record(test, case, ratio)


@pytest.mark.parametrize("n,heads,Nq,Nk", [(2, 2, 192, 192), (1, 5, 300, 77), (1, 2, 33, 130), (4, 10, 2600, 300)])
def test_flash_attention_from_fused_buffers(lib, n, heads, Nq, Nk):
    """flash_attn64: self-attention reads q, k, v as column slices of one [n T, 3C] buffer (runtime_unet.cpp), cross-attention k, v from the
    [n L, 2C] K/V cache (L = 77; 130 and 300 ragged the other way; the last shape triggers the two-query-block form).  Poison rows directly
    behind the last key row: a ragged key tile that loads them and multiplies by a zero probability yields NaN."""
    pb = _attn_problem(n, heads, 64, Nq, Nk, Nq == Nk)
    call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, Nq, Nk, 0.125,
                                                                                        stream_ptr())
    _attn_judge(lib, "flash_attention", "%dx%dx%dx%d" % (n, heads, Nq, Nk), pb, n, heads, 64, Nq, Nk, call)


@pytest.mark.parametrize("kind,n,heads,hd,Nq,Nk", [("flash", 2, 2, 64, 192, 192), ("flash", 1, 5, 64, 300, 77), ("flash", 1, 2, 64, 33, 130),
                                                   ("causal", 2, 2, 64, 77, 77), ("generic", 2, 2, 80, 257, 257)])
def test_attention_small_logits_resolve_a_few_ulps(lib, kind, n, heads, hd, Nq, Nk):
    """Resolution of the attention checks.  attention_ref_bound charges the kernels' fp16 rounding of the pre-scaled query and of the
    probabilities in the worst direction over all keys; at the N(0, 1) inputs of the cases above, where the output is a cancelling average
    (sum p |v| >> |sum p v|), that is 50-100 fp16 ulps of the result: those cases find poison, dropped or doubled keys and wrong tiles, not
    errors of a few ulps.  Here the same layouts run with logits of a few tenths and a positive V (sum p |v| = |ref|), where the derived bound
    is about one ulp at EVERY element: the fp16 probabilities give 2^-11 sum p |v| = 2^-11 |ref| <= ulp16(ref), the score and summation terms
    (logits of a few tenths, at most 300 keys) stay under half an ulp.  Asserted from the reference: the largest bound of the case is under
    1.5 ulps, so the per-element check resolves a few ulps on the real kernels too."""
    pb = _attn_problem(n, heads, hd, Nq, Nk, Nq == Nk, causal=kind == "causal", seed=340, small=True)
    assert float((pb["bound"] / U.ulp16(pb["ref"])).max()) < 1.5
    sc = pb["scale"]
    if kind == "flash":
        call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, Nq, Nk, sc,
                                                                                            stream_ptr())
    elif kind == "causal":
        call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention_causal(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, Nq, Nk,
                                                                                                   sc, 1, stream_ptr())
    else:
        call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention_generic(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, hd,
                                                                                                    Nq, Nk, sc, stream_ptr())
    _attn_judge(lib, "attention_small_logits", "%s-%dx%dx%dx%d" % (kind, n, heads, Nq, Nk), pb, n, heads, hd, Nq, Nk, call)


@pytest.mark.parametrize("T", [77, 200])
def test_flash_attention_causal_from_fused_buffer(lib, T):
    """the CLIP text encoder's causal attention on the fused [n T, 3C] buffer (runtime_text.cpp)"""
    n, heads = 2, 2
    pb = _attn_problem(n, heads, 64, T, T, True, causal=True, seed=240)
    call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention_causal(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, T, T,
                                                                                               0.125, 1, stream_ptr())
    _attn_judge(lib, "flash_attention_causal", "T%d" % T, pb, n, heads, 64, T, T, call)


def test_attention_generic_from_fused_buffer(lib):
    """attn_generic: heads of 80 at 257 tokens from a fused [n T, 3C] buffer (the vision tower's layout)"""
    n, heads, hd, T = 2, 2, 80, 257
    pb = _attn_problem(n, heads, hd, T, T, True, seed=250)
    call = lambda q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so: lib.ladi_op_attention_generic(q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, n, heads, hd, T, T,
                                                                                                pb["scale"], stream_ptr())
    _attn_judge(lib, "attention_generic", "hd80-T257", pb, n, heads, hd, T, T, call)


@pytest.mark.parametrize("hd,T", [(512, 255), (128, 17)])
def test_flash_attention_wide_vae_layout(lib, hd, T):
    """flash_attn_wide in the VAE mid-block's layout (runtime_vae.cpp): q and k are the halves of one [n T, 2C] buffer (ldq = ldk = 2C), V is
    transposed [n][C][ldvt] with ldvt = T rounded up to 4 -- the padding columns and everything behind the last V^T row are poison"""
    n, ldvt = 2, (T + 3) // 4 * 4
    q, k, v = _rand((n, T, hd), 95), _rand((n, T, hd), 96), _rand((n, T, hd), 97)
    k[0, T - 1] *= 3.0                                           # a dominant key in the ragged segment
    scale = 1.0 / math.sqrt(hd)
    ref, bound = U.attention_ref_bound(q, k, v, scale)
    qk = U.guarded(torch.cat([q, k], -1).half(), pre_rows=KV_GUARD, post_rows=KV_GUARD)
    vt = U.guarded(v.half().transpose(1, 2).reshape(n * hd, T), ld=ldvt, pre_rows=4, post_rows=4)
    ldo = hd + 8

    def launch():
        out = U.guarded_out(n * T, hd, ld=ldo, pre_rows=4, post_rows=4)
        rc = lib.ladi_op_attention_wide(qk.col(0), qk.col(hd), vt.ptr, out.ptr, 2 * hd, 2 * hd, ldvt, ldo, T * 2 * hd, T * 2 * hd, hd * ldvt, T * ldo,
                                        n, hd, T, T, scale, stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return out
    out = launch()
    what = "flash_attention_wide hd %d T %d" % (hd, T)
    loc = lambda i: "(sample, query, d) = (%d, %d, %d); last 32-key tile starts at key %d" % (i // hd // T, i // hd % T, i % hd, (T - 1) // 32 * 32)
    ratio = U.check_elem(out.cpu().float(), ref.reshape(n * T, hd), bound.reshape(n * T, hd), what, loc)
    U.assert_untouched(out, what + " output")
    U.assert_untouched(qk, what + " input qk")
    U.assert_untouched(vt, what + " input vt")
    assert torch.equal(launch().cpu(), out.cpu()), what + ": repeat differs"
    _record("flash_attention_wide", "hd%d-T%d" % (hd, T), ratio)


# ---------------------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C,rows", [(512, 77), (512, 4096), (512, 4097), (520, 4096), (520, 4097), (1536, 4097), (1544, 77), (1544, 4099), (4096, 5)])
def test_layer_norm_strided_every_instantiation(lib, C, rows):
    """every layernorm_kernel<R, MAXO> instantiation and both sides of each threshold (norm.hip ladi_launch_layernorm): octets 64 | 65, 192 |
    193, rows 4096 | 4097 (one row per wave | four); 4097 and 4099 leave the last R = 4 wave and the last block partly empty.  Input a view
    with ldx = C + 8, output with ldo = C + 16.  Inputs with mean 1 and sigma 3, like test_gpu_ops.py's test."""
    x, g, b = _rand((rows, C), 36, 3.0) + 1, _rand((C,), 37, 0.1) + 1, _rand((C,), 38, 0.1)
    x, g = x.half().float(), g.half().float()
    ref, bound = U.layer_norm_ref_bound(x, g, b, 1e-5)
    X = U.guarded(x.half(), ld=C + 8, pre_rows=4, post_rows=4)
    G, B = g.half().to(U.dev()), b.half().to(U.dev())

    def launch():
        out = U.guarded_out(rows, C, ld=C + 16, pre_rows=4, post_rows=4)
        assert lib.ladi_op_layer_norm_ld(X.ptr, X.ld, ptr(G), ptr(B), 1e-5, rows, C, out.ptr, out.ld, stream_ptr()) == 0
        torch.cuda.synchronize()
        return out
    out = launch()
    what = "layer_norm C %d rows %d" % (C, rows)
    loc = lambda i: "(row, c) = (%d, %d); block of 16 rows %d / of 4 rows %d" % (i // C, i % C, i // C // 16, i // C // 4)
    ratio = U.check_elem(out.cpu().float(), ref, bound, what, loc)
    U.assert_untouched(out, what + " output")
    U.assert_untouched(X, what + " input")
    assert torch.equal(launch().cpu(), out.cpu()), what + ": repeat differs"
    _record("layer_norm_strided", "C%d-rows%d" % (C, rows), ratio)


def test_layer_norm_ld_agrees_with_the_dense_entry_point(lib):
    """the old entry point stays: dense operands through both give the same bits"""
    rows, C = 77, 320
    x, g, b = _rand((rows, C), 36, 3.0) + 1, _rand((C,), 37, 0.1) + 1, _rand((C,), 38, 0.1)
    X, G, B = x.half().to(U.dev()), g.half().to(U.dev()), b.half().to(U.dev())
    o1, o2 = torch.empty_like(X), torch.empty_like(X)
    assert lib.ladi_op_layer_norm(ptr(X), ptr(G), ptr(B), 1e-5, rows, C, ptr(o1), stream_ptr()) == 0
    assert lib.ladi_op_layer_norm_ld(ptr(X), C, ptr(G), ptr(B), 1e-5, rows, C, ptr(o2), C, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
    assert lib.ladi_op_layer_norm_ld(ptr(X), C + 4, ptr(G), ptr(B), 1e-5, rows, C, ptr(o2), C, stream_ptr()) != 0      # strides are multiples of 8


@functools.lru_cache(maxsize=None)
def _gn_problem(c0, c1, h, w, n, silu):
    a = _rand((n, c0, h, w), 31, 2.0) + 0.5
    b2 = _rand((n, c1, h, w), 32) if c1 else None
    gam, bet = (_rand((c0 + c1,), 33, 0.1) + 1).half().float(), _rand((c0 + c1,), 34, 0.1).half().float()
    add = _rand((n, c0 + c1, h, w), 35)
    xcat = (torch.cat([a, b2], 1) if c1 else a).half().float()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(n * h * w, -1)
    out = {}
    for with_add in (False, True):
        ref, bound = U.group_norm_ref_bound(xcat, 32, gam, bet, 1e-5, silu=bool(silu), add=add if with_add else None)
        out[with_add] = (flat(ref), flat(bound))
    dense = lambda t: U.guarded(t.permute(0, 2, 3, 1).half(), pre_rows=8, post_rows=8)     # EXACTLY the tensor's channels: ld = C
    return dict(A=dense(a), B2=dense(b2) if c1 else None, AD=dense(add), G=gam.half().to(U.dev()), B=bet.half().to(U.dev()), refs=out)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("c0,c1,hw,n,silu", [(320, 0, (64, 48), 2, 1),        # 96 partial rows: the one-pass kernel's limit
                                             (128, 0, (96, 64), 2, 1),        # many partial rows: folded first (gn_reduce_rows)
                                             (96, 32, (8, 6), 2, 0),          # 48-pixel samples: statistics straight from the data
                                             (128, 64, (17, 15), 2, 1),       # HW = 255: not a multiple of 32
                                             (64, 0, (256, 128), 1, 1)])      # HW = 32768: 64 partial rows folded by gn_reduce_rows, then the
                                                                              # one-pass kernel's HW >= 32768 starting block (halved from there to fill the chip)
def test_group_norm_between_poison_rows(lib, c0, c1, hw, n, silu, with_add):
    """ladi_op_group_norm on dense operands (what production passes) between poison rows: sources, the added tensor and the output"""
    h, w = hw
    pb = _gn_problem(c0, c1, h, w, n, silu)
    ref, bound = pb["refs"][with_add]
    Ct = c0 + c1
    stats = torch.empty((n * 32 * 2,), dtype=torch.float32, device=U.dev())

    def launch():
        out = U.guarded_out(n * h * w, Ct, pre_rows=8, post_rows=8)
        rc = lib.ladi_op_group_norm(pb["A"].ptr, c0, pb["B2"].ptr if c1 else None, c1, n, h * w, 32, ptr(pb["G"]), ptr(pb["B"]), 1e-5, silu,
                                    pb["AD"].ptr if with_add else None, out.ptr, ptr(stats), stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return out
    out = launch()
    what = "group_norm (%d | %d) at %dx%d add %d" % (c0, c1, h, w, with_add)
    ratio = U.check_elem(out.cpu().float(), ref, bound, what, U.pixel_locator(n, h, w, Ct))
    U.assert_untouched(out, what + " output")
    for g in (pb["A"], pb["B2"], pb["AD"]):
        if g is not None:
            U.assert_untouched(g, what + " input")
    assert torch.equal(launch().cpu(), out.cpu()), what + ": repeat differs"       # atomics-free, fixed summation order
    _record("group_norm", "%d+%d-%dx%d-add%d" % (c0, c1, h, w, with_add), ratio)


def test_softmax_rows_guarded(lib):
    """ladi_op_softmax_rows at 130 x 192"""
    rows, cols = 130, 192
    s = _rand((rows, cols), 39, 4.0)
    ref, bound = U.softmax_rows_ref_bound(s, 0.3)
    # the entry point takes dense rows (cols is its stride): fp32 scores and fp16 probabilities dense between poison rows
    S = U.guarded(s, pre_rows=4, post_rows=4)
    out = U.guarded_out(rows, cols, pre_rows=4, post_rows=4)
    assert lib.ladi_op_softmax_rows(S.ptr, rows, cols, 0.3, out.ptr, stream_ptr()) == 0
    torch.cuda.synchronize()
    ratio = U.check_elem(out.cpu().float(), ref, bound, "softmax_rows", lambda i: "(row, col) = (%d, %d)" % (i // cols, i % cols))
    U.assert_untouched(out, "softmax_rows output")
    U.assert_untouched(S, "softmax_rows input")
    _record("softmax_rows", "130x192", ratio)
