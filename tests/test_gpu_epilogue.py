"""The epilogue fields and the batched launches that only the VAE, the time embedding, the TPS correlation and the ViT patch embedding use,
per kernel family, judged element by element against float64.

tests/test_gpu_ops.py and tests/test_gpu_views.py launch every implicit-GEMM family with batch = 1, out_scale = 1, bias_mul = 0, no res1, no
per-pixel bias, no rowadd_idx, ldw = 0 and every bs_* stride zero.  The code that handles those fields exists three times (the generic
epilogue, the fast epilogue with its split-K combine, splitk_reduce_kernel) and every family reaches it with its own LDS layout; here each
family runs
  (a) the VAE's fp16 range guard: bias * bias_mul, out_scale, res0 + res1 with different strides (+ mask), also through the scalar stores,
  (b) the same fields through split-K, in-launch combine and two-pass,
  (c) the time-embedding row selected on the device (rowadd_idx / rowadd_stride) out of a table whose other rows are NaN,
  (d) GELU and ReLU,
  (e) batched launches in the callers' layouts, every element in one allocation with poison between the elements,
  (f) the combinations the launcher must refuse without touching the output.
Cases, references and bounds come from tests/epilogue_cases.py (tests/test_cpu_epilogue.py shows on the CPU that the bounds hold for a
faithful epilogue and that every single mistake fails them).  Every operand is a strided view between poison rows (tests/util.py guarded):
a read of a neighbour turns the output NaN, a stray store changes a poison pattern.  The worst err / limit of every judged case goes into
the parity record under "epilogue/..." and "batched/..." keys.

Two refusals under (f) are rules the launcher gained together with this file (ladi_launch_igemm, rc -18 and -19), read off the code:
  * batch > 1 with a second source: igemm_kernel.h and igemm8.hip offset src0 and W by the batch element and never src1, and nothing
    refused the launch; see test_refuses_batched_second_source
  * out_f32 with an activation / rowadd / res0 / res1 / mask: the fp32 branch of igemm_epilogue_generic applies bias and out_scale and
    returns, and nothing refused the launch; see test_refuses_fp32_output_with_an_epilogue"""
import ctypes
import functools

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import stream_ptr
from tests import epilogue_cases as E
from tests import util as U
from tests.test_gpu_views import _cfg_tile, _last_launch

pytestmark = pytest.mark.gpu

FAMILY_OF = {3: "ring", 5: "ring", 7: "ring", 19: "ring", 39: "ring", 14: "ring", 32: "igemm8", 56: "igemm8", 36: "igemm8", 62: "igemm_lc", 69: "igemm_lc",
             74: "halo", 88: "halo", 80: "halo", 109: "halo"}
SPLIT_OF = {14: 2, 36: 2, 69: 2, 80: 2, 109: 8}


def _record(group, test, case, ratio):
    assert ratio <= 1.0, (group, test, case, ratio)
    U.record_parity("%s/%s[%s]" % (group, test, case), round(ratio, 4))


def _poisoned_f32(t):
    """fp32 device copy of t with POISON32 wherever t is NaN"""
    bits = t.contiguous().view(torch.int32).clone()
    bits[torch.isnan(t)] = U.POISON32
    return bits.to(U.dev()).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------- convolutions
class DevConv:
    """the guarded device operands of one tests/epilogue_cases.py ConvCase (built once, launches only read them)"""

    def __init__(self, c):
        self.c = c
        guard = c.w + 2
        g = lambda t, ld: U.guarded(t, ld=ld, pre_rows=guard, post_rows=guard)
        xs = U.nhwc16(c.x)
        self.C0p = xs.shape[3]
        self.X = g(xs, self.C0p + 64)
        self.W = U.pack_conv_weight(c.wt)
        self.B = c.bias.half().to(U.dev())
        self.TE = c.rowadd.float().to(U.dev()) if c.rowadd is not None else None
        self.TAB = _poisoned_f32(c.rowadd_table()) if c.rowadd is not None else None
        self.IDX = torch.tensor([1], dtype=torch.int32, device=U.dev())
        self.R0 = g(E.flat(c.res0).half(), c.ld_res0) if c.res0 is not None else None
        self.R1 = g(E.flat(c.res1).half(), c.ld_res1) if c.res1 is not None else None
        self.M = U.guarded(E.flat(c.mask).reshape(-1, 8).half(), pre_rows=2 * guard, post_rows=2 * guard) if c.mask is not None else None

    def desc(self, out, ldo, table=False):
        c, d = self.c, _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = self.X.ptr, self.C0p, self.X.ld
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = c.h, c.w, c.h, c.w, c.P
        d.ksize, d.stride, d.pad, d.ups = 3, 1, 1, 0
        d.W, d.Q, d.K, d.ldw = self.W.data_ptr(), c.cout, 9 * self.C0p, 0
        d.bias, d.bias_mul, d.act, d.out_scale = self.B.data_ptr(), c.bias_mul, U.ACT[c.act], c.out_scale
        if self.TE is not None and not table:
            d.rowadd = self.TE.data_ptr()
        if self.TE is not None and table:
            d.rowadd, d.rowadd_idx, d.rowadd_stride = self.TAB.data_ptr(), self.IDX.data_ptr(), c.rowadd_stride
        if self.R0 is not None:
            d.res0, d.ldr0 = self.R0.ptr, self.R0.ld
        if self.R1 is not None:
            d.res1, d.ldr1 = self.R1.ptr, self.R1.ld
        if self.M is not None:
            d.mask = self.M.ptr
        d.out, d.ldo = out.ptr, ldo
        return d

    def launch(self, lib, cfg, out_ld=None, table=False):
        ldo = out_ld or self.c.cout + 8
        out = U.guarded_out(self.c.P, self.c.cout, ld=ldo, pre_rows=4, post_rows=4)
        d = self.desc(out, ldo, table)
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
        assert rc == 0, "cfg %d refused the launch: rc = %d (%s)" % (cfg, rc, _lib.last_error())
        torch.cuda.synchronize()
        return out, _last_launch(lib)

    def judge(self, lib, test, cfg, case, out_ld=None, table=False, repeats=0):
        c = self.c
        out, info = self.launch(lib, cfg, out_ld, table)
        bq, bp = _cfg_tile(lib, cfg)
        what = "%s %s %s" % (test, case, info)
        ratio = U.check_elem(out.cpu().float(), c.ref, c.bound, what, U.pixel_locator(c.N, c.h, c.w, c.cout, bq, bp))
        U.assert_untouched(out, what + " output")
        for name, g in (("x", self.X), ("res0", self.R0), ("res1", self.R1), ("mask", self.M)):
            if g is not None:
                U.assert_untouched(g, what + " input " + name)
        first = out.cpu()
        for i in range(repeats):
            again, info2 = self.launch(lib, cfg, out_ld, table)
            assert info2 == info, (what, info2)
            assert torch.equal(again.cpu(), first), "%s: repeat %d differs" % (what, i + 1)
            U.assert_untouched(again, what + " output of repeat %d" % (i + 1))
        assert info["family"] == FAMILY_OF[cfg] and info["split"] == SPLIT_OF.get(cfg, 1), info
        _record("epilogue", test, case, ratio)
        return info


# the float64 references and the guarded device buffers of this file stay for the session (a few MB): every configuration of a case shares them
@functools.lru_cache(maxsize=None)
def _dev_conv(case):
    return DevConv(case)


class _two_pass:
    """both split-K forms: the in-launch combine (default) and the separate reduce pass, restored on the way out"""

    def __init__(self, lib, on):
        self.lib, self.on = lib, on

    def __enter__(self):
        if self.on:
            self.lib.ladi_igemm_set_splitk_two_pass(1)

    def __exit__(self, *exc):
        self.lib.ladi_igemm_set_splitk_two_pass(0)


@pytest.mark.parametrize("out_scale,mask", E.RANGE_GUARD)
@pytest.mark.parametrize("cfg", [3, 7, 19, 39, 32, 56, 62, 74, 88])
def test_range_guard_epilogue(lib, cfg, out_scale, mask):
    """(a) N = 2, 128 -> 320 at 20 x 13: SiLU, a bias of magnitude 1 times bias_mul = 0.125, out_scale 0.125 (the VAE's) and 0.7 (not a power of
    two: the product rounds), res0 at ld = Q + 64 and res1 at ld = Q + 32, the last once more under a mask"""
    _dev_conv(E.range_guard_case(out_scale, mask)).judge(lib, "range_guard", cfg, "cfg%d-os%g-mask%d" % (cfg, out_scale, mask))


@pytest.mark.parametrize("cfg", [3, 32])
def test_range_guard_epilogue_scalar_stores(lib, cfg):
    """the same through the generic epilogue: out_ld = Q + 4 is no multiple of 8, every store is a scalar one and the four columns behind
    every output row are poison that must survive"""
    c = E.range_guard_case(0.7, True)
    _dev_conv(c).judge(lib, "range_guard_scalar_stores", cfg, "cfg%d" % cfg, out_ld=c.cout + 4)


@pytest.mark.parametrize("two_pass", [0, 1])
@pytest.mark.parametrize("cfg", [14, 36, 69, 80, 109])
def test_range_guard_epilogue_split_k(lib, cfg, two_pass):
    """(b) N = 2, 512 -> 192 at 8 x 6 with SiLU, the time-embedding row, bias_mul, out_scale, res0 and res1 through every family's split-K
    representative, in both forms: the in-launch combine (the fused epilogues) and the separate pass (splitk_reduce_kernel); five bit-equal
    repeats of each"""
    with _two_pass(lib, two_pass):
        _dev_conv(E.deep_k_case("silu")).judge(lib, "split_k", cfg, "cfg%d-%s" % (cfg, "two_pass" if two_pass else "in_launch"), repeats=5)


@pytest.mark.parametrize("cfg,two_pass", [(3, 0), (74, 0), (14, 0), (14, 1)])
def test_rowadd_row_selected_on_the_device(lib, cfg, two_pass):
    """(c) the UNet's time embedding: rowadd is an fp32 table [3][Q + 8], a device int holds 1; rows 0 and 2 and the padding columns are NaN,
    so a wrong row or a wrong stride turns the output NaN"""
    with _two_pass(lib, two_pass):
        _dev_conv(E.deep_k_case("silu")).judge(lib, "rowadd_idx", cfg, "cfg%d-%s" % (cfg, "two_pass" if two_pass else "in_launch"), table=True)


@pytest.mark.parametrize("cfg", [3, 32, 74, 14])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_gelu_and_relu(lib, act, cfg):
    """(d) LADI_ACT_GELU against the exact-erf F.gelu in float64 (the allowance for the library's erf polynomial is util.GELU_ERF_ABS), and ReLU"""
    _dev_conv(E.deep_k_case(act)).judge(lib, "activation", cfg, "%s-cfg%d" % (act, cfg))


# ---------------------------------------------------------------------------------------------------------------------- batched GEMMs
class DevBatch:
    """the guarded device operands of one BatchCase: an operand with a batch stride in ONE allocation with poison rows between its elements
    (util.guarded_batch), a shared one as a plain guarded view"""

    def __init__(self, c):
        self.c = c
        place = lambda ts, ld: U.guarded_batch([t.half() for t in ts], ld=ld) if len(ts) > 1 else U.guarded(ts[0].half(), ld=ld)
        if c.qk:
            self.X = self.Wt = place([torch.cat([x, w], -1) for x, w in zip(c.x, c.w)], c.ld0)
            self.src0, self.w = self.X.ptr, self.X.col(c.K)
        else:
            self.X, self.Wt = place(c.x, c.ld0), place(c.w, c.ldw or c.K)
            self.src0, self.w = self.X.ptr, self.Wt.ptr
        self.Bv = c.bias.half().to(U.dev()) if c.bias is not None else None
        self.R = place(c.res, c.ldr) if c.res is not None else None

    def launch(self, lib, cfg):
        """returns (rc, output, bits of the output's allocation before the launch)"""
        c = self.c
        nan = torch.full((c.P, c.Q), float("nan"), dtype=torch.float32 if c.out_f32 else torch.float16)
        out = U.guarded_batch([nan] * c.B, ld=c.ldo, pre_rows=4, post_rows=4)
        before = out._bits().clone()
        d = _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = self.src0, c.K, c.ld0
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = c.P, 1, c.P, 1, c.P
        d.ksize, d.stride, d.pad, d.ups = 1, 1, 0, 0
        d.W, d.Q, d.K, d.ldw = self.w, c.Q, c.K, c.ldw
        d.bs_src0, d.bs_w, d.bs_out = getattr(self.X, "bs", 0), getattr(self.Wt, "bs", 0), out.bs
        if self.Bv is not None:
            d.bias, d.bias_per_pixel = self.Bv.data_ptr(), int(c.bias_per_pixel)
        if self.R is not None:
            d.res0, d.ldr0, d.bs_res = self.R.ptr, self.R.ld, getattr(self.R, "bs", 0)
        d.act, d.out_scale = U.ACT["none"], 1.0
        d.out, d.ldo, d.out_f32 = out.ptr, c.ldo, int(c.out_f32)
        rc = lib.ladi_op_igemm(ctypes.byref(d), c.B, cfg, stream_ptr())
        torch.cuda.synchronize()
        return rc, out, before

    def inputs_untouched(self, what):
        for name, g in (("x", self.X), ("w", self.Wt), ("res", self.R)):
            if g is not None:
                U.assert_untouched(g, what + " input " + name)


@functools.lru_cache(maxsize=None)
def _dev_batch(name):
    return DevBatch(E.batch_case(name))


def _bk64_refuses(name):
    return E.batch_case(name).K % 64 != 0


@pytest.mark.parametrize("cfg", [0, 3, 5, 32])
@pytest.mark.parametrize("name", E.BATCH_CASES)
def test_batched_gemm(lib, name, cfg):
    """(e) batch = 3 in the layouts of the four callers (runtime_vae.cpp V^T / scores / PV, runtime_vision.cpp patch embedding, and a residual
    per element): shared operands at stride 0, a weight operand at ldw > K, q and k as column slices of one buffer, an fp32 output, a
    per-pixel bias, an ldo that is only a multiple of 4, K % 64 != 0.  cfg 0 is the launcher's own choice with the measured selection
    switched off (the cost model is what is judged and nothing is timed inside a test), 3 and 5 two ring tiles, 32 igemm8 -- a BK = 64 tile,
    which must refuse the K = 160 case"""
    db, c = _dev_batch(name), E.batch_case(name)
    if cfg == 0:
        lib.ladi_igemm_set_autotune(0)
    try:
        rc, out, before = db.launch(lib, cfg)
    finally:
        if cfg == 0:
            lib.ladi_igemm_set_autotune(1)
    what = "batched %s cfg %d" % (name, cfg)
    if cfg == 32 and _bk64_refuses(name):
        assert rc != 0 and torch.equal(out._bits(), before), (what, rc)
        return
    assert rc == 0, "%s refused: rc = %d (%s)" % (what, rc, _lib.last_error())
    info = _last_launch(lib)
    loc = lambda i: "(element, row, column) = (%d, %d, %d)" % (i // (c.P * c.Q), i // c.Q % c.P, i % c.Q)
    ratio = U.check_elem(out.cpu().float(), c.ref, c.bound, "%s %s" % (what, info), loc, out_f32=c.out_f32)
    U.assert_untouched(out, what + " output (the rows between the elements included)")
    db.inputs_untouched(what)
    if cfg:
        assert info["family"] == FAMILY_OF[cfg], info
    _record("batched", name, "cfg%d" % cfg, ratio)


def test_batched_gemm_bk64_refuses_k160(lib):
    """cfg 7 (BK = 64) on the PV case: C0 = 160 is no multiple of 64 -- refused, the output untouched"""
    rc, out, before = _dev_batch("vae_pv").launch(lib, 7)
    assert rc != 0 and torch.equal(out._bits(), before), rc


# ---------------------------------------------------------------------------------------------------------------------- refusals
class Refusal:
    """a small problem every tiled family accepts as it stands (N = 1, 128 (+ 64) -> 128 at 8 x 6, 3 x 3), with room for batch = 3 behind
    every operand, and a 1 x 1 one the X-stationary kernel accepts (320 -> 320 at 16 x 16); refused(...) applies one change and expects a
    refusal that leaves the poisoned output bit-identical"""

    def __init__(self, xs=False):
        self.xs = xs
        self.h, self.w, self.cin, self.cout, self.k = (16, 16, 320, 320, 1) if xs else (8, 6, 128, 128, 3)
        self.P = self.h * self.w
        el = lambda shape, seed: [E.rand(shape, seed + b).half() for b in range(3)]
        self.X = U.guarded_batch(el((self.P, self.cin), 700), ld=self.cin + 64, gap_rows=self.w + 2, pre_rows=self.w + 2, post_rows=self.w + 2)
        self.X1 = U.guarded_batch(el((self.P, 64), 710), ld=128, gap_rows=self.w + 2, pre_rows=self.w + 2, post_rows=self.w + 2)
        self.W = E.rand((self.cout, self.k * self.k * (self.cin + 64)), 720, 0.03).half().to(U.dev())
        self.B = E.rand((max(self.cout, self.P),), 721).half().to(U.dev())
        self.TE = E.rand((self.cout,), 722).to(U.dev())
        self.R = U.guarded_batch(el((self.P, self.cout), 730), ld=self.cout + 8)
        self.M = torch.zeros((self.P,), dtype=torch.float16, device=U.dev())

    def desc(self, out, batch=1, src1=False, **fields):
        d = _lib.IGemmDesc()
        d.src0, d.C0, d.ld0 = self.X.ptr, self.cin, self.X.ld
        c1 = 64 if src1 else 0
        if src1:
            d.src1, d.C1, d.ld1 = self.X1.ptr, 64, self.X1.ld
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = self.h, self.w, self.h, self.w, self.P
        d.ksize, d.stride, d.pad, d.ups = self.k, 1, self.k // 2, 0
        d.W, d.Q, d.K, d.ldw = self.W.data_ptr(), self.cout, self.k * self.k * (self.cin + c1), 0       # ldw = 0: rows K apart
        d.bias, d.act, d.out_scale = self.B.data_ptr(), U.ACT["none"], 1.0
        d.out, d.ldo = out.ptr, out.ld
        if batch > 1:
            d.bs_src0, d.bs_out, d.bs_res = self.X.bs, out.bs, self.R.bs
        for k, v in fields.items():
            if k in ("res0", "res1"):
                setattr(d, k, self.R.ptr)
                setattr(d, "ldr" + k[-1], self.R.ld)
            elif k == "rowadd":
                d.rowadd = self.TE.data_ptr()
            elif k == "mask":
                d.mask = self.M.data_ptr()
            elif k == "act":
                d.act = U.ACT[v]
            else:
                setattr(d, k, v)
        return d

    def refused(self, lib, cfg, batch=1, src1=False, **fields):
        nan = torch.full((self.P, self.cout), float("nan"), dtype=torch.float32 if fields.get("out_f32") else torch.float16)
        out = U.guarded_batch([nan] * 3, ld=self.cout + 8, pre_rows=4, post_rows=4)
        before = out._bits().clone()
        d = self.desc(out, batch, src1, **fields)
        rc = lib.ladi_op_igemm(ctypes.byref(d), batch, cfg, stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0, "cfg %d batch %d src1 %d %r: the launch was not refused" % (cfg, batch, src1, fields)
        assert torch.equal(out._bits(), before), "cfg %d batch %d src1 %d %r: refused with rc = %d, but the output changed" % (cfg, batch, src1, fields, rc)
        return rc

    def accepted(self, lib, cfg):
        """the unchanged problem runs on cfg: what refused() adds is the only reason for its refusals"""
        out = U.guarded_out(self.P, self.cout, ld=self.cout + 8, pre_rows=4, post_rows=4)
        d = self.desc(out)
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (cfg, rc, _lib.last_error())
        assert bool(torch.isfinite(out.cpu().float()).all())
        U.assert_untouched(out, "refusal baseline cfg %d" % cfg)
        return _last_launch(lib)


@functools.lru_cache(maxsize=None)
def _refusal(xs=False):
    return Refusal(xs)


@pytest.fixture
def cost_model(lib):
    """cfg 0 without the measured selection: nothing is timed inside a test"""
    lib.ladi_igemm_set_autotune(0)
    try:
        yield
    finally:
        lib.ladi_igemm_set_autotune(1)


@pytest.mark.parametrize("cfg", [0, 3, 32])
def test_refuses_batched_second_source(lib, cost_model, cfg):
    """batch > 1 with src1 / C1: the kernels offset src0 and W by the batch element and never src1 (there is no bs_src1), so every element
    would read element 0's second source.  Before the launcher refused it (rc -18), this launch returned 0."""
    assert _refusal().refused(lib, cfg, batch=3, src1=True) == -18


@pytest.mark.parametrize("cfg", [0, 3])
@pytest.mark.parametrize("field,value", [("act", "silu"), ("act", "gelu"), ("act", "relu"), ("rowadd", 1), ("res0", 1), ("res1", 1), ("mask", 1)])
def test_refuses_fp32_output_with_an_epilogue(lib, cost_model, cfg, field, value):
    """out_f32 stores (acc + bias * bias_mul) * out_scale and returns: an activation, rowadd, a residual or a mask would be dropped silently.
    Before the launcher refused them (rc -19), each of these launches returned 0 and stored the value without the field."""
    assert _refusal().refused(lib, cfg, out_f32=1, **{field: value}) == -19


def test_fp32_output_with_bias_and_scale_alone_still_runs(lib):
    """what the fp32 store does implement stays accepted (the VAE's score product is such a launch)"""
    r = _refusal()
    out = U.guarded_out(r.P, r.cout, ld=r.cout + 8, pre_rows=4, post_rows=4, dtype=torch.float32)
    d = _lib.IGemmDesc()
    d.src0, d.C0, d.ld0 = r.X.ptr, r.cin, r.X.ld
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = r.h, r.w, r.h, r.w, r.P
    d.ksize, d.stride, d.pad = 3, 1, 1
    d.W, d.Q, d.K = r.W.data_ptr(), r.cout, 9 * r.cin
    d.bias, d.bias_mul, d.out_scale = r.B.data_ptr(), 0.5, 0.25
    d.out, d.ldo, d.out_f32 = out.ptr, out.ld, 1
    assert lib.ladi_op_igemm(ctypes.byref(d), 1, 3, stream_ptr()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    x = r.X.views[0].cpu().float().reshape(1, r.h, r.w, r.cin).permute(0, 3, 1, 2)
    wt = r.W.cpu().float().flatten()[:r.cout * 9 * r.cin].reshape(r.cout, 9, r.cin).permute(0, 2, 1).reshape(r.cout, r.cin, 3, 3)   # ldw = 0: rows K apart
    ref, bound = U.conv_ref_bound(x, wt, bias=r.B.cpu().float()[:r.cout], bias_mul=0.5, out_scale=0.25)
    ratio = U.check_elem(out.cpu(), E.flat(ref), E.flat(bound), "fp32 output, bias * 0.5, out_scale 0.25", out_f32=True)
    U.assert_untouched(out, "fp32 output")
    _record("epilogue", "fp32_bias_scale", "cfg3", ratio)


@pytest.mark.parametrize("cfg,family", [(62, "igemm_lc"), (74, "halo"), (14, "ring")])
def test_refuses_batched_launch_on_unbatched_kernels(lib, cfg, family):
    """the loader / consumer kernel, the halo kernel and every split-K form take batch = 1 only"""
    r = _refusal()
    assert r.accepted(lib, cfg)["family"] == family
    r.refused(lib, cfg, batch=3)


def test_refuses_batched_launch_on_the_x_stationary_kernel(lib):
    r = _refusal(xs=True)
    assert r.accepted(lib, 25)["family"] == "linear_xs"
    r.refused(lib, 25, batch=3)


@pytest.mark.parametrize("fields", [dict(bias_per_pixel=1), dict(out_f32=1)])
def test_split_k_refuses_per_pixel_bias_and_fp32_output(lib, fields):
    r = _refusal()
    assert r.accepted(lib, 14)["split"] == 2
    r.refused(lib, 14, **fields)


@pytest.mark.parametrize("fields", [dict(out_scale=0.5), dict(bias_mul=0.5), dict(res1=1)])
def test_x_stationary_kernel_refuses_the_range_guard_fields(lib, fields):
    """linear_xs implements bias, one residual, GEGLU and the fused norms: no out_scale, no bias_mul, no second residual"""
    r = _refusal(xs=True)
    assert r.accepted(lib, 25)["family"] == "linear_xs"
    r.refused(lib, 25, **fields)
