"""The cases of tests/test_gpu_epilogue.py as CPU data, and an fp32 emulation of the kernels' arithmetic with switchable mistakes.

Every case holds its operands (fp32 tensors of fp16-representable values), the float64 reference and the derived bound (tests/util.py
conv_ref_bound / gemm_batched_ref_bound).  tests/test_gpu_epilogue.py places the operands in poisoned device buffers and judges the
kernels; tests/test_cpu_epilogue.py judges emulate_conv() / emulate_batched() with the same check_elem and the same bounds: the faithful
emulation must pass (the reference alone stays inside its bound), every mutant -- one mistake an epilogue could make -- must fail (the
inputs are lively enough for the check to see it)."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import util as U

NAN = float("nan")


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def f32(v):
    """the value an fp32 descriptor field holds"""
    return float(torch.tensor(v, dtype=torch.float32))


def flat(t):
    """[N, C, H, W] -> pixel rows [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---------------------------------------------------------------------------------------------------------------------- convolutions
class ConvCase:
    """a 3x3 pad-1 stride-1 convolution with the whole epilogue: bias (magnitude about 1) * bias_mul, time-embedding row (bare, and as row 1
    of a [3][Q + 8] table whose other rows and padding columns are NaN), activation, out_scale, two residuals with different row strides
    (ld_res0 / ld_res1: the device placement and the emulation's wrong-stride mutant use them), mask"""

    def __init__(self, N, cin, cout, h, w, act="silu", seed=400, bias_mul=1.0, out_scale=1.0, rowadd=False, res0=True, res1=False, mask=False):
        self.N, self.cin, self.cout, self.h, self.w, self.act = N, cin, cout, h, w, act
        self.bias_mul, self.out_scale = bias_mul, out_scale
        self.P = N * h * w
        self.x = rand((N, cin, h, w), seed)
        self.wt = rand((cout, cin, 3, 3), seed + 1, 1 / math.sqrt(9 * cin))
        self.bias = rand((cout,), seed + 2)
        self.rowadd = rand((cout,), seed + 3) if rowadd else None
        self.res0 = rand((N, cout, h, w), seed + 4) if res0 else None
        self.res1 = rand((N, cout, h, w), seed + 5) if res1 else None
        self.mask = (torch.rand((N, 1, h, w), generator=torch.Generator().manual_seed(seed + 6)) > 0.5).float() if mask else None
        self.ld_res0, self.ld_res1 = cout + 64, cout + 32
        self.rowadd_stride = cout + 8
        ref, bound = U.conv_ref_bound(self.x, self.wt, bias=self.bias, rowadd=self.rowadd, act=act, res=self.res0, mask=self.mask,
                                      bias_mul=f32(bias_mul), out_scale=f32(out_scale), res1=self.res1)
        self.ref, self.bound = flat(ref), flat(bound)

    def rowadd_table(self):
        """fp32 [3][Q + 8]: row 1 the time-embedding row, everything else NaN (the device copy carries POISON32 there)"""
        t = torch.full((3, self.rowadd_stride), NAN)
        t[1, :self.cout] = self.rowadd
        return t


@functools.lru_cache(maxsize=None)
def range_guard_case(out_scale, mask):
    """section (a): N = 2, 128 -> 320 at 20 x 13 (780 pixels, ragged against every tile): SiLU, bias * 0.125, out_scale, res0 + res1 (+ mask)"""
    return ConvCase(2, 128, 320, 20, 13, act="silu", seed=400 + int(out_scale * 1000) + (7 if mask else 0), bias_mul=0.125, out_scale=out_scale,
                    res1=True, mask=mask)


RANGE_GUARD = [(0.125, False), (0.7, False), (0.7, True)]


@functools.lru_cache(maxsize=None)
def deep_k_case(act="silu"):
    """sections (b) - (d): N = 2, 512 -> 192 at 8 x 6 (few tiles, 72 K tiles: every split-K form is at home).  SiLU: every field of the range
    guard plus the time-embedding row; GELU / ReLU: bias + residual"""
    if act == "silu":
        return ConvCase(2, 512, 192, 8, 6, act="silu", seed=500, bias_mul=0.125, out_scale=0.7, rowadd=True, res1=True)
    return ConvCase(2, 512, 192, 8, 6, act=act, seed=510 + len(act))


def _act32(v, act):
    return dict(none=lambda t: t, relu=F.relu, silu=F.silu, gelu=F.gelu)[act](v)


def _strided_rows(t, ld):
    """[P, C] -> the flat buffer a device view with row stride ld occupies (padding columns NaN, one spare row so that a wrong stride stays inside)"""
    P, C = t.shape
    buf = torch.full(((P + 1) * max(ld, C) * 2,), NAN)
    buf.as_strided((P, C), (ld, 1)).copy_(t)
    return buf


CONV_MUTANTS = ("bias_mul_dropped", "bias_mul_on_rowadd", "out_scale_after_residual", "out_scale_twice", "res1_skipped", "res1_read_with_ldr0",
                "wrong_rowadd_row")


def emulate_conv(c, mutant=None, rowadd_from_table=False):
    """the epilogue's arithmetic in torch fp32: fp16 operands, fp32 accumulation, bias * bias_mul rounded to fp32, the sum, the activation in
    fp32, ONE rounding of t * out_scale to fp16, the residuals added in fp32, the mask, the final fp16 rounding.  Returns [P, Q] fp16."""
    assert mutant is None or mutant in CONV_MUTANTS
    s = flat(F.conv2d(c.x, c.wt, padding=1))                                  # fp32 accumulation of exact products
    bm, osc = torch.tensor(c.bias_mul, dtype=torch.float32), torch.tensor(c.out_scale, dtype=torch.float32)
    v = s + (c.bias if mutant == "bias_mul_dropped" else c.bias * bm)
    if c.rowadd is not None:
        ra = c.rowadd
        if rowadd_from_table or mutant == "wrong_rowadd_row":
            ra = c.rowadd_table()[0 if mutant == "wrong_rowadd_row" else 1, :c.cout]
        v = v + (ra * bm if mutant == "bias_mul_on_rowadd" else ra)
    t = _act32(v, c.act)
    late = mutant == "out_scale_after_residual"
    y = (t if late else t * osc * (osc if mutant == "out_scale_twice" else 1.0)).half().float()
    if c.res0 is not None:
        y = y + flat(c.res0)
    if c.res1 is not None and mutant != "res1_skipped":
        r1 = flat(c.res1)
        if mutant == "res1_read_with_ldr0":
            r1 = _strided_rows(r1, c.ld_res1).as_strided(r1.shape, (c.ld_res0, 1))
        y = y + r1
    if late:
        y = y * osc
    if c.mask is not None:
        y = y * (1.0 - flat(c.mask))
    return y.half()


# ---------------------------------------------------------------------------------------------------------------------- batched GEMMs
class BatchCase:
    """a batched launch of the linear form, batch = 3: out[b] = x[b] w[b]^T + bias (+ res[b]).  x / w / res are lists of 3 tensors, or of one
    for a shared operand (batch stride 0); ld0 / ldw / ldo / ldr the row strides of the device placement; qk: x and w are the column halves
    of one buffer per element (ld0 = ldw = 2 K, W = src0 + K)"""

    def __init__(self, name, x, w, ld0, ldw, ldo, bias=None, bias_per_pixel=False, res=None, ldr=0, out_f32=False, qk=False):
        self.name, self.x, self.w, self.bias, self.bias_per_pixel, self.res, self.out_f32, self.qk = name, x, w, bias, bias_per_pixel, res, out_f32, qk
        self.B, self.P, self.K, self.Q = 3, x[0].shape[0], x[0].shape[1], w[0].shape[0]
        self.ld0, self.ldw, self.ldo, self.ldr = ld0, ldw, ldo, ldr
        self.ref, self.bound = U.gemm_batched_ref_bound(x, w, bias=bias, bias_per_pixel=bias_per_pixel, res=res, out_f32=out_f32)
        for i in range(3):
            for j in range(i):          # all three elements differ: a launch that computes element 0 three times cannot pass
                assert float((self.ref[i] - self.ref[j]).abs().mean()) > 0.1 * float(self.ref[i].abs().mean()), (name, i, j)


BATCH_CASES = ("vae_vt", "vae_scores", "vae_pv", "vit_patch_embed", "batched_residual")


@functools.lru_cache(maxsize=None)
def batch_case(name):
    el = lambda shape, seed, scale=1.0: [rand(shape, seed + 10 * b, scale) for b in range(3)]       # a different seed per element
    if name == "vae_vt":             # V^T[b] = Wv Xn[b]^T + bv: the pixel operand is the SHARED weight, the weight operand the tokens at ldw = 128
        return BatchCase(name, [rand((64, 64), 600, 0.125)], el((100, 64), 601), ld0=64, ldw=128, ldo=100, bias=rand((64,), 602), bias_per_pixel=True)
    if name == "vae_scores":         # S[b] = Q[b] K[b]^T in fp32, q and k the column halves of one [160][256] buffer
        return BatchCase(name, el((160, 128), 610, 0.3), el((160, 128), 611, 0.3), ld0=256, ldw=256, ldo=160, out_f32=True, qk=True)
    if name == "vae_pv":             # O[b] = P[b] V[b] with K = T = 160 (K % 64 != 0): probabilities times V^T rows at ldw = 160
        p = [torch.softmax(v, -1).half().float() for v in el((160, 160), 620, 2.0)]
        return BatchCase(name, p, el((64, 160), 621), ld0=168, ldw=160, ldo=72)
    if name == "vit_patch_embed":    # patch rows x SHARED weight + bias + the SHARED position embedding as the residual
        return BatchCase(name, el((50, 192), 630), [rand((96, 192), 631, 1 / math.sqrt(192))], ld0=256, ldw=0, ldo=112, bias=rand((96,), 632),
                         res=[rand((50, 96), 633)], ldr=104)
    if name == "batched_residual":   # the same with a residual per element (bs_res != 0, and != bs_out)
        return BatchCase(name, el((50, 192), 630), [rand((96, 192), 631, 1 / math.sqrt(192))], ld0=256, ldw=0, ldo=112, bias=rand((96,), 632),
                         res=el((50, 96), 634), ldr=104)
    raise KeyError(name)


BATCH_MUTANTS = ("pixel_bias_by_channel", "batch_reads_element0", "bs_res_for_bs_out")
GAP = 3      # poison rows between two batch elements of the emulation's output (tests/util.py guarded_batch on the device)


def emulate_batched(c, mutant=None):
    """the batched launch in torch fp32, written through the strides a launch uses: element z's output lands z * bs_out elements behind
    element 0's in a NaN-filled buffer (an element the launch never wrote stays NaN).  Returns [B, P, Q] in the output's dtype."""
    assert mutant is None or mutant in BATCH_MUTANTS
    bs_out = (c.P + GAP) * c.ldo
    bs_res = (c.P + GAP) * c.ldr if c.res is not None and len(c.res) > 1 else 0
    odt = torch.float32 if c.out_f32 else torch.float16
    buf = torch.full((c.B * max(bs_out, bs_res) + bs_out,), NAN, dtype=odt)
    for z in range(c.B):
        zz = 0 if mutant == "batch_reads_element0" else z
        s = c.x[zz % len(c.x)] @ c.w[zz % len(c.w)].t()                        # fp32 accumulation of exact products
        if c.bias is not None:
            if c.bias_per_pixel and mutant != "pixel_bias_by_channel":
                s = s + c.bias[:, None]
            else:
                s = s + c.bias[torch.arange(c.Q) % c.bias.numel()][None, :]
        if c.res is not None:
            s = s.half().float() + c.res[zz % len(c.res)]
        off = z * (bs_res if mutant == "bs_res_for_bs_out" else bs_out)
        buf.as_strided((c.P, c.Q), (c.ldo, 1), off).copy_(s.to(odt))
    return torch.stack([buf.as_strided((c.P, c.Q), (c.ldo, 1), z * bs_out) for z in range(c.B)])
