"""Shared helpers for the parity tests (HIP path called through the C ABI vs the CPU oracle / plain torch fp32)."""
import ctypes
import math

import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import IGemmDesc, ptr, stream_ptr

ACT = dict(none=0, silu=1, gelu=2, geglu=3, relu=4, tanh=5)


def dev():
    return torch.device("cuda", 0)


def nhwc16(x):
    """[N,C,H,W] fp32 cpu -> NHWC fp16 on the GPU, channels zero-padded to a multiple of 64"""
    n, c, h, w = x.shape
    cp = (c + 63) // 64 * 64
    out = torch.zeros((n, h, w, cp), dtype=torch.float16)
    out[..., :c] = x.permute(0, 2, 3, 1).half()
    return out.to(dev())


def pack_conv_weight(w):
    """[cout,cin,k,k] -> [cout, k*k, cin_pad] fp16 (tap-major, channel-minor; the igemm layout)"""
    co, ci, k, _ = w.shape
    cp = (ci + 63) // 64 * 64
    out = torch.zeros((co, k * k, cp), dtype=torch.float16)
    out[:, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, k * k, ci).half()
    return out.reshape(co, k * k * cp).contiguous().to(dev())


def igemm(x, w_packed, cout, ksize=3, stride=1, pad=None, ups=0, x2=None, bias=None, rowadd=None, act="none", res0=None, res1=None,
          mask=None, out_f32=False, cfg=0, out_ld=None, ln=None, gn=None):
    """x, x2: NHWC fp16 gpu tensors [N,H,W,C]; returns NHWC output [N,Ho,Wo,ldo]"""
    lib = _lib.load()
    N, H, W, C0 = x.shape
    C1 = x2.shape[3] if x2 is not None else 0
    Hl, Wl = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (Hl, Wl) if stride == 1 else (Hl // 2, Wl // 2)
    qout = cout // 2 if act == "geglu" else cout
    ldo = out_ld or qout
    out = torch.zeros((N, Ho, Wo, ldo), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    d = IGemmDesc()
    d.src0, d.C0, d.ld0 = x.data_ptr(), C0, C0
    if x2 is not None:
        d.src1, d.C1, d.ld1 = x2.data_ptr(), C1, C1
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = H, W, Ho, Wo, N * Ho * Wo
    d.ksize, d.stride, d.pad, d.ups = ksize, stride, (ksize // 2 if pad is None else pad), ups
    d.W, d.Q, d.K, d.ldw = w_packed.data_ptr(), cout, ksize * ksize * (C0 + C1), 0
    keep = []
    if bias is not None:
        b = bias.half().to(x.device); keep.append(b); d.bias = b.data_ptr()
    if rowadd is not None:
        r = rowadd.float().to(x.device); keep.append(r); d.rowadd = r.data_ptr()
    d.act, d.out_scale = ACT[act], 1.0
    if res0 is not None:
        d.res0, d.ldr0 = res0.data_ptr(), res0.shape[3]
    if res1 is not None:
        d.res1, d.ldr1 = res1.data_ptr(), res1.shape[3]
    if mask is not None:
        d.mask = mask.data_ptr()
    if ln is not None:       # (gamma, beta, eps[, with_scratch]): LayerNorm of the pixel operand (fused, or via the scratch)
        gm, bt = ln[0].half().to(x.device), ln[1].half().to(x.device)
        keep += [gm, bt]
        d.ln_gamma, d.ln_beta, d.ln_eps = gm.data_ptr(), bt.data_ptr(), float(ln[2])
        if len(ln) > 3 and ln[3]:
            scr = torch.empty((x.shape[0] * x.shape[1] * x.shape[2], x.shape[3]), dtype=torch.float16, device=x.device)
            keep.append(scr)
            d.ln_scratch = scr.data_ptr()
    if gn is not None:       # (scale_shift [n][C0][2] fp32 gpu tensor, pixels per sample): GroupNorm affine of the pixel operand
        keep.append(gn[0])
        d.gn_ss, d.gn_hw = gn[0].data_ptr(), int(gn[1])
    d.out, d.ldo, d.out_f32 = out.data_ptr(), ldo, int(out_f32)
    rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
    assert rc == 0, "igemm rc=%d %s" % (rc, _lib.last_error())
    torch.cuda.synchronize()
    return out


def to_nchw(y, c=None):
    y = y.float().cpu().permute(0, 3, 1, 2)
    return y[:, :c] if c is not None else y


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def psnr(a, b, peak=None):
    a, b = a.double(), b.double()
    peak = float(b.abs().max()) if peak is None else peak
    mse = float(((a - b) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def cpu_quota_threads():
    """usable host threads: min(affinity, cgroup cpu.max quota) — torch oversubscribes badly when it sees 256 logical CPUs
    but the container is capped (the GPU box: quota 16 of 256)"""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(int(q) / int(p))))
    except Exception:
        pass
    return n


PARITY_NAME = "parity_r06.json"


def library_digest():
    """sha256 over the sources / headers / flags libladi_native.so is built from (ladi_vton_amd/build.py: the stamp the loader checks)"""
    from ladi_vton_amd import build
    return build._digest()


def parity_path():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(os.environ.get("GRAFT_REPO_ROOT", root), "gpurun_out", PARITY_NAME)


def record_parity(key, value, name=None):
    """Measured parity values of the GPU suite -> gpurun_out/parity_r06.json (the only directory that comes back from the GPU box), stamped
    with the library digest and the pytest session id: tests/conftest.py removes the file at the start of every GPU session, so the record
    is ONE run of ONE binary, never a stitch.  `python tools/commit_parity.py` copies it to profiles/r06_parity.json after
    checking the digest against the sources; tests/test_cpu.py checks that every key the documents cite is in the committed file."""
    import json
    import os
    path = parity_path() if name is None else os.path.join(os.path.dirname(parity_path()), name)
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        blob = json.load(open(path)) if os.path.exists(path) else {}
        blob["_library_digest"] = library_digest()
        blob.setdefault("_session", os.environ.get("LADI_PYTEST_SESSION", ""))
        blob[key] = value
        json.dump(blob, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


# ----------------------------------------------------------------------------------------------------------------------------------------
# Strided, offset views with poisoned surroundings (tests/test_gpu_views.py, tests/test_cpu_views.py)
#
# The product hands every kernel views into a bump arena: q / k / v are column slices of the fused QKV buffer, convolutions write into
# out_ld 4 / 8 buffers and into caller views, LayerNorm runs on x.ld.  guarded() reproduces that placement for one operand and fills
# everything the contract (include/ladi_native.h) says the kernel does not use with NaN, assert_untouched() checks that a launch left every
# such element bit-identical, and check_elem() judges the result element by element against a float64 reference.
# ----------------------------------------------------------------------------------------------------------------------------------------
POISON16 = 0x7E5A                   # an fp16 quiet NaN with a payload no arithmetic produces
POISON32 = 0x7FC5A5A5               # the same for fp32


class Guarded:
    """one operand inside its poisoned allocation: .buf the whole 1-D device buffer, .view the [rows, C] strided device view of the operand
    (row stride .ld elements), .ptr its address, .pre / .post the poison rows before / after it"""

    def __init__(self, buf, rows, C, ld, pre, post):
        self.buf, self.rows, self.C, self.ld, self.pre, self.post = buf, rows, C, ld, pre, post
        self.view = buf.as_strided((rows, C), (ld, 1), pre * ld)
        self.ptr = self.view.data_ptr()

    def col(self, c0):
        """address of column c0 of the view's first row (q / k / v slices of a fused buffer)"""
        return self.ptr + c0 * self.buf.element_size()

    def cpu(self):
        return self.view.cpu()

    def _bits(self):
        return self.buf.view(torch.int16 if self.buf.dtype == torch.float16 else torch.int32).cpu()

    def poison_mask(self):
        """bool [pre + rows + post, ld]: True where the allocation holds poison (outside the view)"""
        m = torch.ones((self.pre + self.rows + self.post, self.ld), dtype=torch.bool)
        m[self.pre:self.pre + self.rows, :self.C] = False
        return m


def _poison_word(dtype):
    # the int16 / int32 value with the poison's bit pattern (two's complement for the sign-less patterns above: both are < 2^15 / 2^31)
    return (torch.int16, POISON16) if dtype == torch.float16 else (torch.int32, POISON32)


def guarded(t, ld=None, pre_rows=2, post_rows=2, device=None, any_ld=False):
    """Place an fp16 / fp32 operand t ([rows, C], or NHWC [N, H, W, C] flattened to pixel rows; CPU or GPU) inside a larger device buffer of
    NaN: pre_rows rows of poison, then the rows of t at row stride ld (default C: dense), columns [C, ld) of every row poison, then post_rows
    rows of poison.  ld % 8 == 0 (ld % 4 == 0 is accepted for the two strides the ABI itself defines that way: out_ld = 4 of the UNet's output
    layer and the V^T rows of the wide attention) and pre_rows rounded up to the next count that puts the view on a 16-byte boundary of the
    torch allocator's 256-byte aligned block, as every launcher requires.
    What t itself holds is the caller's business: channel padding the contract defines as ZERO (nhwc16's padding to 64, packed-weight padding)
    is part of t and stays zero.  device: default the GPU ("cpu" for the harness's own CPU test).  any_ld: accept a stride that is no multiple
    of 4 (the helper kernels that address element by element: an fp32 output of 3 channels at ld = 3, dense buffers of odd length).
    Returns a Guarded."""
    assert t.dtype in (torch.float16, torch.float32)
    t2 = t.reshape(-1, t.shape[-1])
    rows, C = t2.shape
    ld = C if ld is None else ld
    assert ld >= C and (ld % 4 == 0 or any_ld), (C, ld)
    while (pre_rows * ld * t.element_size()) % 16:
        pre_rows += 1
    it, word = _poison_word(t.dtype)
    device = dev() if device is None else torch.device(device)
    buf = torch.full(((pre_rows + rows + post_rows) * ld,), word, dtype=it, device=device).view(t.dtype)
    g = Guarded(buf, rows, C, ld, pre_rows, post_rows)
    g.view.copy_(t2.to(device))
    assert g.ptr % 16 == 0
    return g


class GuardedBatch(Guarded):
    """B operands of a batched launch in ONE poisoned allocation: element b is the [erows, C] view .views[b] at row stride ld, .bs elements
    (erows + gap rows) behind element b - 1 -- the rows between two elements are poison like the rows before the first and after the last, so
    a wrong batch stride reads NaN or overwrites a poison pattern.  .ptr is element 0's address, .rows the span from element 0's first row to
    the last element's last row (what assert_untouched walks)."""

    def __init__(self, buf, B, erows, C, ld, gap, pre, post):
        self.B, self.erows, self.gap, self.bs = B, erows, gap, (erows + gap) * ld
        super().__init__(buf, B * erows + (B - 1) * gap, C, ld, pre, post)
        self.views = [buf.as_strided((erows, C), (ld, 1), pre * ld + b * self.bs) for b in range(B)]
        self.view = None

    def cpu(self):
        return torch.stack([v.cpu() for v in self.views])

    def poison_mask(self):
        m = torch.ones((self.pre + self.rows + self.post, self.ld), dtype=torch.bool)
        for b in range(self.B):
            r0 = self.pre + b * (self.erows + self.gap)
            m[r0:r0 + self.erows, :self.C] = False
        return m


def guarded_batch(ts, ld=None, gap_rows=3, pre_rows=2, post_rows=2, device=None):
    """guarded() for the B same-shaped [rows, C] operands ts of a batched launch (see GuardedBatch).  gap_rows is rounded up to the next count
    that keeps the batch stride a multiple of 8 elements (16 bytes of fp16), as the product's strides are."""
    t0 = ts[0]
    assert t0.dtype in (torch.float16, torch.float32) and all(t.shape == t0.shape and t.dtype == t0.dtype for t in ts)
    erows, C = t0.shape
    ld = C if ld is None else ld
    assert ld >= C and ld % 4 == 0 and gap_rows >= 1, (C, ld)
    while ((erows + gap_rows) * ld) % 8:
        gap_rows += 1
    while (pre_rows * ld * t0.element_size()) % 16:
        pre_rows += 1
    it, word = _poison_word(t0.dtype)
    device = dev() if device is None else torch.device(device)
    B = len(ts)
    buf = torch.full(((pre_rows + B * erows + (B - 1) * gap_rows + post_rows) * ld,), word, dtype=it, device=device).view(t0.dtype)
    g = GuardedBatch(buf, B, erows, C, ld, gap_rows, pre_rows, post_rows)
    for v, t in zip(g.views, ts):
        v.copy_(t.to(device))
    assert g.ptr % 16 == 0
    return g


def guarded_out(rows, C, ld=None, pre_rows=2, post_rows=2, dtype=torch.float16, device=None, any_ld=False):
    """an OUTPUT placed like guarded(): the view itself starts as NaN too, so an element the kernel never wrote fails check_elem"""
    return guarded(torch.full((rows, C), float("nan"), dtype=dtype), ld, pre_rows, post_rows, device, any_ld)


def assert_untouched(g, what=""):
    """every poison element of g's allocation is still bit-identical (raw 16 / 32-bit patterns: NaN != NaN)"""
    _, word = _poison_word(g.buf.dtype)
    bits = g._bits().reshape(g.pre + g.rows + g.post, g.ld)
    bad = (bits != word) & g.poison_mask()
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d poison elements were overwritten; first at allocation row %d (view row %d of %d), column %d (C = %d, ld = %d): "
                             "bits 0x%X" % (what, int(bad.sum()), r, r - g.pre, g.rows, c, g.C, g.ld, int(bits[r, c]) & (0xFFFF if g.buf.dtype == torch.float16 else 0xFFFFFFFF)))


# ----------------------------------------------------------------------------------------------------------------------------------------
# Far views (tests/far_cases.py, tests/test_gpu_far.py, tests/test_cpu_far.py): the same placement at row strides of megabytes, so that a
# problem of a few hundred rows spans more than 2^31 or 2^32 bytes.  Only the allocation is large: the operand stays [rows, C].  Nothing
# here copies the allocation to the host or builds a host tensor that grows with the span -- the poison is counted on the device, in chunks.
# ----------------------------------------------------------------------------------------------------------------------------------------
FAR_PAD = 4096                      # poison elements in front of the first and behind the last operand element (a multiple of 8)
FAR_CHUNK = 1 << 26                 # elements compared per step of the poison count: a 64 MiB bool temporary at most


class FarGuarded:
    """one operand of n samples x srows rows x C columns inside ONE poisoned 1-D allocation .buf: row r of sample s starts at element
    .pad + s * sstride + r * ld.  .views[s] is the [srows, C] strided device view of sample s (.view = .views[0] when n == 1), .ptr the address
    of the first element, .bytes the allocation's size, .last_byte the byte offset (from .ptr) of the operand's last element."""

    def __init__(self, buf, n, srows, C, ld, sstride, pad):
        self.buf, self.n, self.srows, self.C, self.ld, self.sstride, self.pad = buf, n, srows, C, ld, sstride, pad
        self.rows = n * srows
        self.views = [buf.as_strided((srows, C), (ld, 1), pad + s * sstride) for s in range(n)]
        self.view = self.views[0] if n == 1 else None
        self.ptr = self.views[0].data_ptr()
        self.bytes = buf.numel() * buf.element_size()
        self.last_byte = ((n - 1) * sstride + (srows - 1) * ld + C) * buf.element_size() - 1

    def col(self, c0):
        return self.ptr + c0 * self.buf.element_size()

    def cpu(self):
        """the operand's values, [n * srows, C], on the host (the views only: rows x C elements)"""
        return torch.cat([v.cpu() for v in self.views])

    def inside(self, idx):
        """bool tensor: which of the flat allocation indices idx (int64 tensor) belong to the operand"""
        rel = idx - self.pad
        s = torch.div(rel, self.sstride, rounding_mode="floor") if self.n > 1 else torch.zeros_like(rel)
        s = s.clamp(0, self.n - 1)
        within = rel - s * self.sstride
        r, c = torch.div(within, self.ld, rounding_mode="floor"), within % self.ld
        return (rel >= 0) & (r >= 0) & (r < self.srows) & (c < self.C)


def guarded_far(t, ld, samples=1, sstride=None, device=None):
    """guarded() for wide strides: the fp16 / fp32 operand t ([rows, C], or NHWC flattened to pixel rows; CPU or GPU) placed at row stride ld
    elements, its rows split into `samples` equal groups that lie sstride elements apart (default: srows * ld, i.e. one uniform row stride;
    a per-sample or batch stride otherwise -- at least (srows - 1) * ld + C so that samples do not overlap).  Everything else of the
    allocation -- FAR_PAD elements before and after, the columns [C, ld) of every row, the gaps between samples -- holds POISON16 / POISON32.
    ld and sstride are multiples of 8 (16-byte aligned rows of fp16, as every launcher requires).  Returns a FarGuarded."""
    assert t.dtype in (torch.float16, torch.float32)
    t2 = t.reshape(-1, t.shape[-1])
    rows, C = t2.shape
    assert rows % samples == 0, (rows, samples)
    srows = rows // samples
    sstride = srows * ld if sstride is None else sstride
    assert ld >= C and ld % 8 == 0 and sstride % 8 == 0 and (samples == 1 or sstride >= (srows - 1) * ld + C), (C, ld, sstride)
    it, word = _poison_word(t.dtype)
    device = dev() if device is None else torch.device(device)
    total = FAR_PAD + (samples - 1) * sstride + (srows - 1) * ld + C + FAR_PAD
    buf = torch.full((total,), word, dtype=it, device=device).view(t.dtype)
    g = FarGuarded(buf, samples, srows, C, ld, sstride, FAR_PAD)
    for s, v in enumerate(g.views):
        v.copy_(t2[s * srows:(s + 1) * srows].to(device))
    assert g.ptr % 16 == 0
    return g


def guarded_far_out(rows, C, ld, samples=1, sstride=None, dtype=torch.float16, device=None):
    """an OUTPUT placed like guarded_far(): the operand itself starts as NaN (not the poison pattern), so an element the kernel never wrote
    fails check_elem"""
    return guarded_far(torch.full((rows, C), float("nan"), dtype=dtype), ld, samples, sstride, device)


def far_stray_count(g):
    """number of elements of g's allocation OUTSIDE the operand that no longer hold the poison pattern, counted where the allocation lives:
    the raw words that differ from the poison are counted chunk by chunk over the whole allocation, and those inside the operand (rows x C
    elements, gathered through the views) are subtracted.  One scalar reaches the host."""
    it, word = _poison_word(g.buf.dtype)
    bits = g.buf.view(it)
    total = torch.zeros((), dtype=torch.int64, device=bits.device)
    for c0 in range(0, bits.numel(), FAR_CHUNK):
        total += (bits[c0:c0 + FAR_CHUNK] != word).sum()
    for v in g.views:
        total -= (v.view(it) != word).sum()
    return int(total)


def assert_untouched_far(g, what=""):
    """assert_untouched() for a FarGuarded: every poison element of the allocation is still bit-identical.  The count runs on the device
    (far_stray_count); only after a failure are the first strays located, chunk by chunk, for the message."""
    n = far_stray_count(g)
    if n == 0:
        return
    it, word = _poison_word(g.buf.dtype)
    bits = g.buf.view(it)
    found = []
    for c0 in range(0, bits.numel(), FAR_CHUNK):
        idx = (bits[c0:c0 + FAR_CHUNK] != word).nonzero().reshape(-1) + c0
        idx = idx[~g.inside(idx)][:4]
        found += [(int(i), int(bits[int(i)]) & (0xFFFF if g.buf.dtype == torch.float16 else 0xFFFFFFFF)) for i in idx]
        if len(found) >= 4:
            break
    raise AssertionError("%s: %d poison elements were overwritten; first at allocation elements %s (operand: %d samples x %d rows x %d columns at "
                         "element %d, ld = %d, sample stride = %d)" % (what, n, ", ".join("%d (bits 0x%X)" % f for f in found), g.n, g.srows, g.C,
                                                                       g.pad, g.ld, g.sstride))


U16 = 2.0 ** -11       # unit roundoff of fp16 (round to nearest): |fp16(x) - x| <= U16 |x| for normal x
U32 = 2.0 ** -24       # unit roundoff of fp32


def ulp16(x):
    """spacing of fp16 numbers at |x| (float64 tensor): 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range.  Rounding a real to fp16
    moves it by at most half of this; check_elem grants one whole spacing so that a reference a hair below a binade boundary does not halve
    the allowance of a result a hair above it."""
    a = x.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10.0)


def check_elem(got, ref, bound, what, locate=None, out_f32=False):
    """Per-element check |got - ref| <= ulp16(ref) + bound.  got: the kernel's output (any float dtype, CPU), ref: float64 reference,
    bound: float64 tensor (or scalar) >= 0 derived from the reference alone (the *_bound helpers below) for everything between the exact
    result and the value that is finally rounded to fp16.  A non-finite output element fails by itself.  locate(flat_index) -> str names
    the failing element for the message (pixel, channel, tile).  Returns the worst err / (ulp16(ref) + bound), the margin the tests record.
    out_f32: the kernel stores fp32 -- the final rounding is an fp32 one, so U32 |ref| takes the place of ulp16(ref) (the messages keep
    calling that term "ulp16")."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert bool(torch.isfinite(ref).all()) and bool((bound >= 0).all()), what
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        i = int((~fin).reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d non-finite output elements; first at flat index %d %s: got %r, ref %.6g"
                             % (what, int((~fin).sum()), i, locate(i) if locate else "", float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))
    err = (got - ref).abs()
    last = U32 * ref.abs() if out_f32 else ulp16(ref)
    lim = last + bound
    ratio = err / lim
    bad = err > lim
    if bool(bad.any()):
        i = int(torch.where(bad.reshape(-1), ratio.reshape(-1), torch.zeros(())).argmax())
        f = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside ulp16(ref) + bound; first at flat index %d %s; worst at %d %s: got %.6g, ref %.6g, "
                             "err %.3g, limit %.3g (ulp16 %.3g + bound %.3g)"
                             % (what, int(bad.sum()), bad.numel(), f, locate(f) if locate else "", i, locate(i) if locate else "",
                                float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(err.reshape(-1)[i]), float(lim.reshape(-1)[i]),
                                float(last.reshape(-1)[i]), float(bound.reshape(-1)[i])))
    return float(ratio.max())


# Lipschitz constants of the epilogue's activations (sup |f'|): SiLU 1.0999 at x = 2.3994, exact GELU 1.1290 at x = sqrt(2), ReLU / none 1,
# tanh 1 at x = 0
ACT_LIP = dict(none=1.0, relu=1.0, silu=1.1, gelu=1.13, tanh=1.0)
# fp32 evaluation of an activation with the hardware's fast exp / reciprocal (v_exp_f32 and v_rcp_f32 are specified to 1 ulp, the erf / tanh
# polynomial a few more): 16 fp32 ulps of the result, a documented allowance, not a measurement
ACT_EVAL = 16.0 * U32
GELU_ERF_ABS = 1.5e-7               # |error| of the erf approximation the library's gelu_f uses (Abramowitz & Stegun 7.1.26, csrc/common.h): an
                                    # ABSOLUTE error of erf, so gelu(x) = x (1 + erf(x / sqrt 2)) / 2 carries |x| GELU_ERF_ABS / 2 on top


def _act_eval_err(x, t, act):
    """error of evaluating t = act(x) in fp32 (x exact)"""
    if act == "none":
        return torch.zeros_like(t)
    e = ACT_EVAL * t.abs()
    return e + 0.5 * GELU_ERF_ABS * x.abs() if act == "gelu" else e


def _act64(x, act):
    import torch.nn.functional as F
    return dict(none=lambda v: v, relu=F.relu, silu=F.silu, gelu=F.gelu, tanh=torch.tanh)[act](x)


def conv_ref_bound(x, w, bias=None, rowadd=None, act="none", res=None, mask=None, stride=1, padding=1, x_err=None,
                   bias_mul=1.0, out_scale=1.0, res1=None, bias_per_pixel=False):
    """float64 reference and the derived error bound of ladi_op_igemm's convolution / linear epilogue
        t   = act(conv(x, w) + bias * bias_mul + rowadd)          (bias [Q] by channel, or [N, 1, Ho, Wo] by pixel when bias_per_pixel)
        out = fp16( fp16(t * out_scale) + res + res1 ) * (1 - mask)
    x [N, C, H, W] (already padded / upsampled as the case needs), w [Q, C, k, k], all values fp16-representable.

    Derivation (u = 2^-24, the fp32 unit roundoff).  The kernels accumulate the K = C k k products in fp32; products of two fp16 values are
    exact in fp32, so the only error of s = conv(x, w) is the summation's.  For ANY order of an fp32 sum of K terms the running-error bound is
        |fl(s) - s| <= K u (|w| (*) |x|)                                  (Higham, Accuracy and Stability, eq. 4.4 with gamma_K ~ K u),
    where |w| (*) |x| is the same convolution applied to absolute values -- computed here by the same float64 code.  bias and rowadd are
    added in fp32: two more roundings of a value no larger than A = |w| (*) |x| + |bias| + |rowadd|, so e_pre = (K + 2) u A.
    An operand the kernel first normalises and rounds to fp16 (fused LayerNorm / GroupNorm affine) enters with a per-element perturbation
    x_err >= 0 (same shape as x); it reaches the sum as |w| (*) x_err, added to e_pre.
    The activation f propagates e_pre by its Lipschitz constant (ACT_LIP) and is itself evaluated in fp32 with fast intrinsics:
    e_act = L e_pre + ACT_EVAL |f|.  Without a residual that is the whole bound: the one fp16 rounding left is check_elem's ulp16(ref).
    With a residual the epilogue rounds t = f(...) to fp16 BEFORE the residual is added in fp32 (the rounding point of every epilogue of the
    library: igemm_common.h step (1) / (2)), so the bound gains half an ulp16 for that rounding -- evaluated at |t| + e_act so that
    the binade of the computed t is covered -- plus one fp32 rounding of the sum, u |ref|.  The mask multiplies by exactly 0 or 1.

    The VAE's range-guard fields (each term vanishes at the field's neutral value, where the operation is exact in fp32):
      bias_mul   the product bias * bias_mul is formed in fp32 before it is added: one more rounding, u |bias bias_mul|; the sum and its
                 magnitude A carry the product
      out_scale  t * out_scale is one fp32 product, rounded to fp16 at once: the error of t is scaled by |out_scale| and the product adds
                 u |t out_scale| (zero when out_scale is a power of two -- the general term is kept); the half-ulp16 of the pre-residual
                 rounding is taken at |t out_scale| + e
      res1       a second residual is one further fp32 add: u |t out_scale + res| for the first sum as before, u (|ref| + e) for the second,
                 whose left operand is the computed first sum
    Returns (ref, bound), float64 [N, Q, Ho, Wo]."""
    import torch.nn.functional as F
    x, w = x.double(), w.double()
    K = w.shape[1] * w.shape[2] * w.shape[3]
    s = F.conv2d(x, w, stride=stride, padding=padding)
    e = torch.zeros_like(s)
    xa = x.abs()
    if x_err is not None:
        e = e + F.conv2d(x_err.double(), w.abs(), stride=stride, padding=padding)
        xa = xa + x_err.double()                      # the summation bound is over the operand the kernel actually multiplies
    A = F.conv2d(xa, w.abs(), stride=stride, padding=padding)
    if bias is not None:
        b = bias.double() * float(bias_mul)
        b = b.reshape(s.shape[0], 1, s.shape[2], s.shape[3]) if bias_per_pixel else b[None, :, None, None]
        s, A = s + b, A + b.abs()
        if float(bias_mul) != 1.0:
            e = e + U32 * b.abs()
    if rowadd is not None:
        s = s + rowadd.double()[None, :, None, None]
        A = A + rowadd.double().abs()[None, :, None, None]
    e = e + (K + 2) * U32 * A
    t = _act64(s, act)
    e = ACT_LIP[act] * e + _act_eval_err(s, t, act)
    if float(out_scale) != 1.0:
        t = t * float(out_scale)
        e = abs(float(out_scale)) * e + U32 * t.abs()
    ref = t
    if res is not None or res1 is not None:
        e = e + 0.5 * ulp16(t.abs() + e)
        if res is not None:
            ref = ref + res.double()
            e = e + U32 * ref.abs()
        if res1 is not None:
            ref = ref + res1.double()
            e = e + U32 * (ref.abs() + e)
    if mask is not None:
        ref = ref * (1.0 - mask.double())
        e = e * (1.0 - mask.double())
    return ref, e


def geglu_ref_bound(x, w, b, x_err=None):
    """out = (u + bu) * gelu(g + bg) with (u | g) = x w^T, x [T, C], w [2 Qh, C] (torch order: value rows, then gate rows), float64.
    Both halves carry the summation bound of conv_ref_bound, e = (K + 2) u (|w| |x| + |b|) (+ |w| x_err); the product rule gives
        |d(u gelu(g))| <= |gelu(g)| e_u + |u| d_g + e_u d_g,  d_g = L e_g + (evaluation error of gelu),  and one fp32 rounding of the product, u |ref|."""
    import torch.nn.functional as F
    x, w, b = x.double(), w.double(), b.double()
    K = x.shape[1]
    s = x @ w.t() + b
    e = (K + 2) * U32 * (x.abs() @ w.abs().t() + b.abs())
    if x_err is not None:
        e = e + x_err.double() @ w.abs().t()
    (u, g), (eu, eg) = s.chunk(2, -1), e.chunk(2, -1)
    gl = F.gelu(g)
    dg = ACT_LIP["gelu"] * eg + _act_eval_err(g, gl, "gelu")
    ref = u * gl
    return ref, gl.abs() * eu + u.abs() * dg + eu * dg + U32 * ref.abs()


def gemm_batched_ref_bound(x, w, bias=None, bias_per_pixel=False, res=None, out_f32=False):
    """float64 reference and bound of a batched launch of the linear form (ladi_op_igemm with batch = B, ksize 1):
        out[b] = x[b] w[b]^T + bias (+ res[b]),   x[b] [P, K] (the pixel operand), w[b] [Q, K], out[b] [P, Q]
    x / w / res are lists of B tensors, or of ONE tensor for an operand every element shares (its batch stride is 0); bias is [Q], or [P] when
    bias_per_pixel, and always shared.  Every element is conv_ref_bound's 1 x 1 case: the same (K + 2) u (|w| |x| + |bias|) summation bound
    and, with a residual, the same pre-residual rounding.  out_f32: the launch stores the fp32 sum itself -- there is no fp16 rounding, the
    bound is the summation's alone and check_elem(out_f32=True) grants U32 |ref| for the stored value in place of ulp16(ref).
    Returns (ref, bound), float64 [B, P, Q]."""
    B = max(len(x), len(w), len(res) if res is not None else 1)
    assert all(len(v) in (1, B) for v in (x, w) + ((res,) if res is not None else ())) and not (out_f32 and res is not None)
    refs, bounds = [], []
    for b in range(B):
        xb, wb = x[b % len(x)], w[b % len(w)]
        P, K = xb.shape
        Q = wb.shape[0]
        rb = res[b % len(res)].t().reshape(1, Q, P, 1) if res is not None else None
        bb = bias.reshape(1, 1, P, 1) if (bias is not None and bias_per_pixel) else bias
        r, e = conv_ref_bound(xb.t().reshape(1, K, P, 1), wb.reshape(Q, K, 1, 1), bias=bb, bias_per_pixel=bias_per_pixel, res=rb, padding=0)
        refs.append(r.reshape(Q, P).t())
        bounds.append(e.reshape(Q, P).t())
    return torch.stack(refs), torch.stack(bounds)


def layer_norm_ref_bound(x, gamma, beta, eps):
    """float64 LayerNorm over the last dimension and the bound of an fp32 implementation (any summation order).
    With C terms: mean m = sum(x) / C carries e_m = (C + 1) u mean|x|; the variance is computed either as mean((x - m)^2) or as
    mean(x^2) - m^2 -- the second form is the worse one and is what is bounded: e_v = (C + 3) u mean(x^2) + 2 |m| e_m  (the inputs of the
    tests have mean 1 and sigma 3, which keeps mean(x^2) / var at 10 / 9 and this term harmless).  r = rsqrt(v + eps):
    |dr| <= r e_v / (2 (v + eps)) + 2 u r (v_rsq_f32 is specified to 1 ulp).  y = (x - m) r gamma + beta:
        |dy| <= |gamma| (e_m r + |x - m| |dr|) + 4 u (|(x - m) r gamma| + |beta|)      (four fp32 roundings: subtract, two products, add)
    The single fp16 rounding of y is check_elem's ulp16(ref)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    C = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    e_m = (C + 1) * U32 * x.abs().mean(-1, keepdim=True)
    e_v = (C + 3) * U32 * (x * x).mean(-1, keepdim=True) + 2 * m.abs() * e_m
    r = torch.rsqrt(v + eps)
    dr = r * e_v / (2 * (v + eps)) + 2 * U32 * r
    core = (x - m) * r * gamma
    ref = core + beta
    bound = gamma.abs() * (e_m * r + (x - m).abs() * dr) + 4 * U32 * (core.abs() + beta.abs())
    return ref, bound


def group_norm_ref_bound(x, groups, gamma, beta, eps, silu=False, add=None):
    """float64 GroupNorm (+ SiLU) (+ add) of x [N, C, H, W] and the bound of the library's form: per-channel partial sums in fp32, group
    statistics from them, the affine y = x scale + shift with scale = r gamma, shift = beta - m r gamma in fp32, SiLU, `add` in fp32 (one more
    fp32 rounding, u |ref|), ONE rounding to fp16 (norm.hip gn_apply_kernel / gn_norm_kernel).  n = pixels x channels of a group; statistics as in
    layer_norm_ref_bound with C -> n (E[x^2] - m^2 form); the shift's cancellation is covered by bounding |x scale| and |shift| separately:
        |dy| <= |x| |dscale| + |dshift| + 2 u (|x scale| + |shift|),  dscale = |gamma| |dr| + u |scale|,
        dshift = |gamma| (e_m r + |m| |dr|) + 3 u (|m r gamma| + |beta|)."""
    import torch.nn.functional as F
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    N, C, H, W = x.shape
    xg = x.reshape(N, groups, -1)
    n = xg.shape[-1]
    m = xg.mean(-1, keepdim=True)
    v = ((xg - m) ** 2).mean(-1, keepdim=True)
    e_m = (n + 1) * U32 * xg.abs().mean(-1, keepdim=True)
    e_v = (n + 3) * U32 * (xg * xg).mean(-1, keepdim=True) + 2 * m.abs() * e_m
    r = torch.rsqrt(v + eps)
    dr = r * e_v / (2 * (v + eps)) + 2 * U32 * r
    per_ch = lambda t: t.expand(N, groups, C // groups).reshape(N, C, 1, 1)
    m, r, e_m, dr = per_ch(m), per_ch(r), per_ch(e_m), per_ch(dr)
    g4, b4 = gamma.reshape(1, C, 1, 1), beta.reshape(1, C, 1, 1)
    scale, shift = r * g4, b4 - m * r * g4
    y = x * scale + shift
    dscale = g4.abs() * dr + U32 * scale.abs()
    dshift = g4.abs() * (e_m * r + m.abs() * dr) + 3 * U32 * ((m * r * g4).abs() + b4.abs())
    e = x.abs() * dscale + dshift + 2 * U32 * ((x * scale).abs() + shift.abs())
    if silu:
        t = F.silu(y)
        e = ACT_LIP["silu"] * e + ACT_EVAL * t.abs()
        y = t
    if add is not None:
        ref = y + add.double()
        e = e + U32 * ref.abs()
        y = ref
    return y, e


def stats_rows_ref_bound(stored, n, HW):
    """float64 per-sample, per-channel statistics of a STORED fp16 output -- stored: float64 [n HW, Q] pixel rows holding fp16-representable
    values -- and the bound of an fp32 accumulation of them in ANY order: what the partial rows an igemm epilogue writes for the consuming
    GroupNorm must add up to.  The unit is the sample: rows [s rps, (s + 1) rps) of a producer's buffer belong to sample s, and that is all
    the three readers (gn_norm, gn_reduce, gn_finalize: norm.hip) rely on, so a producer is judged on the float64 sum of its fp32 rows per
    sample (an exact combine of fp32 partial sums is one more summation order, and the most favourable one).

    Derivation (u = 2^-24).  Every term of the sum is an fp16 value, exact in fp32.  For ANY order of an fp32 sum of HW terms the running-
    error bound is |fl(S) - S| <= gamma_(HW - 1) sum|v| (Higham, Accuracy and Stability, eq. 4.4), gamma_k = k u / (1 - k u): granted as
        HW u sum|v|                                                               for the sum,
    which exceeds gamma_(HW - 1) while HW u < 1 / HW, i.e. for every HW up to 4096 pixels per sample; above that gamma_(HW - 1) itself is
    granted.  The square of an fp16 value has at most 22 significant bits and an exponent of at least -48: exact in fp32 as well, so
    the sum of squares is the same kind of sum.  Its terms are granted one rounding each all the same (an implementation is free to form
    them with a rounded multiply-add), and one further unit covers the second-order terms of gamma_(HW + 1):
        (HW + 2) u sum v^2                                                        for the sum of squares.
    Statistics of the UNROUNDED fp32 value differ from those of the stored fp16 value by the HW final roundings, each up to 2^-11 |v| and of
    either sign: about sqrt(HW / 3) 2^-11 rms(v) for the sum, against a bound of HW u sum|v| ~ 0.8 HW^2 u rms(v) -- a ratio of about
    6000 / HW^1.5, i.e. 0.8 at the 384 pixels per sample of the suite and less above.  That is less than this bound resolves: rows taken
    before the final rounding would pass or fail by the luck of the signs, and nothing is asserted about that difference.  What the bound
    does resolve is a row credited to the wrong sample, a missing or doubled block of pixels, and statistics taken before the residual add or
    the mask (tests/test_cpu_stats_ref.py plants each of them).
    Returns (sum, sumsq, bound_sum, bound_sumsq), float64 [n, Q] each."""
    v = stored.double().reshape(n, HW, -1)
    assert bool(torch.isfinite(v).all()) and bool((v == v.half().double()).all()), "the stored output must hold finite fp16 values"
    if HW <= 4096:
        return v.sum(1), (v * v).sum(1), HW * U32 * v.abs().sum(1), (HW + 2) * U32 * (v * v).sum(1)
    # samples of more than 4096 pixels (the VAE levels of tests/test_gpu_tuned.py): HW u no longer stands in for gamma_(HW - 1), so gamma itself
    # is granted -- gamma_(HW - 1) for the sum and, by the same count of one rounding per term and two more, gamma_(HW + 1) for the squares
    assert (HW + 1) * U32 < 0.5
    gamma = lambda k: k * U32 / (1.0 - k * U32)
    return v.sum(1), (v * v).sum(1), gamma(HW - 1) * v.abs().sum(1), gamma(HW + 1) * (v * v).sum(1)


def attention_ref_bound(q, k, v, scale, causal=False):
    """float64 softmax(scale q k^T) v for q [.., Nq, d], k, v [.., Nk, d] (leading dims = samples x heads) and the bound of the library's
    flash kernels (attention.hip), whose arithmetic is: q' = fp16(q scale log2 e) -- ONE rounding of the pre-scaled query, relative 2^-11
    per element --, scores q' k in fp32 (d terms), p~ = exp2(s - m_run) in fp32 with m_run within a few units of the row maximum, p~ rounded
    to fp16 for the second product, the denominator summed in fp32 from the unrounded p~, o = (sum p~ v) / l in fp32 (Nk terms), one
    rounding to fp16 (check_elem's ulp16(ref)).
      score error (natural units), per query i and key j:  D_ij = (2^-11 + (d + 2) u) scale sum_c |q_ic| |k_jc|  (the fp16 query + the fp32 sum)
      softmax:  p'_j = p_j e^(d_j) / sum_i p_i e^(d_i) with |d_j| <= D_ij; by Jensen sum_i p_i e^(-D_i) >= e^(-Dbar), Dbar = sum_i p_i D_i, so
                |p'_j - p_j| <= p_j (e^(D_ij + Dbar_i) - 1): a key with a large score error but no weight does not loosen the bound
      fp16 p~:  relative 2^-11 while p~ is normal; below 2^-14 the absolute error is 2^-25, against a denominator l >= 1/2 (the row maximum has
                p~ > 1/2 after the last rescale) -- an absolute 2^-24 per key
      sums:     (Nk + 2) u relative on numerator and denominator each, exp2 to 2 fp32 ulps
        |do_c| <= sum_j p_j (e^(D_ij + Dbar_i) - 1) |v_jc| + (2^-11 + (2 Nk + 8) u) sum_j p_j |v_jc| + 2^-24 sum_j |v_jc|"""
    if q.dim() == 4 and q.shape[0] > 1:             # sample by sample: the float64 score matrices of a large case stay small
        parts = [attention_ref_bound(q[i:i + 1], k[i:i + 1], v[i:i + 1], scale, causal) for i in range(q.shape[0])]
        return torch.cat([r for r, _ in parts]), torch.cat([b for _, b in parts])
    q, k, v = q.double(), k.double(), v.double()
    d, Nk = q.shape[-1], k.shape[-2]
    s = (q @ k.transpose(-1, -2)) * scale
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    if causal:
        keep = torch.ones(s.shape[-2:], dtype=torch.bool).tril()
        s = s.masked_fill(~keep, float("-inf"))
        sa = sa.masked_fill(~keep, 0.0)
    p = torch.softmax(s, -1)
    D = (U16 + (d + 2) * U32) * sa
    Dbar = (p * D).sum(-1, keepdim=True)
    va = v.abs()
    vsum = va.sum(-2, keepdim=True) if not causal else torch.cumsum(va, -2)
    bound = (p * torch.expm1(D + Dbar)) @ va + (U16 + (2 * Nk + 8) * U32) * (p @ va) + 2.0 ** -24 * vsum
    return p @ v, bound


def single_query_ref_bound(q, k, v, scale):
    """float64 softmax(scale q k^T) v for ONE query per (sample, head) -- q [.., d], k, v [.., Nk, d] -- and the bound of the library's
    single-query kernel (attention.hip attn_single_query_kernel): scores s_j = fl(sum_c q_c k_jc) scale in fp32 (products of two fp16 values
    are exact, d terms, one product with the scale), w_j = exp(s_j - m) with m the maximum of the computed scores, numerator sum_j w_j v_j and
    denominator sum_j w_j summed in fp32 over the Nk keys in order, o = numerator * (1 / denominator), one rounding to fp16 (check_elem's ulp16).
      score:   |ds_j| <= (d + 1) u scale sum_c |q_c| |k_jc|; the argument of the exponential adds the rounding of s_j - m and of its product
               with log2 e inside the fast exponential, each u |s_j - m| <= u (|s_j| + max |s|), a third one granted:
                   D_j = (d + 1) u scale sum_c |q_c| |k_jc| + 3 u (|s_j| + max_i |s_i|)
      exp:     evaluated to ACT_EVAL relative, so w~_j = w_j (1 + delta_j), |delta_j| <= eps_j = e^(D_j) (1 + ACT_EVAL) - 1.  Whatever m is, it
               cancels in the quotient, and with p = softmax(s)
                   o~ - o = sum_j p_j delta_j (v_j - o) / (1 + sum_j p_j delta_j),   |o~ - o| <= sum_j p_j eps_j |v_j - o| / (1 - sum_j p_j eps_j):
               a key with a large score error but no weight, or a value equal to the output, does not loosen the bound
      sums:    an Nk-term fp32 sum of rounded products for the numerator, an Nk-term sum for the denominator, the reciprocal and the final
               product: (2 Nk + 6) u sum_j p_j |v_j|
    Returns (ref, bound), float64 [.., d]."""
    q, k, v = q.double(), k.double(), v.double()
    d, Nk = q.shape[-1], k.shape[-2]
    s = (k @ q.unsqueeze(-1)).squeeze(-1) * scale                     # [.., Nk]
    sa = (k.abs() @ q.abs().unsqueeze(-1)).squeeze(-1) * abs(scale)
    p = torch.softmax(s, -1)
    D = (d + 1) * U32 * sa + 3 * U32 * (s.abs() + s.abs().amax(-1, keepdim=True))
    eps = torch.exp(D) * (1.0 + ACT_EVAL) - 1.0
    ref = (p.unsqueeze(-2) @ v).squeeze(-2)                           # [.., d]
    pe = p * eps
    num = (pe.unsqueeze(-2) @ (v - ref.unsqueeze(-2)).abs()).squeeze(-2)
    bound = num / (1.0 - pe.sum(-1, keepdim=True)) + (2 * Nk + 6) * U32 * (p.unsqueeze(-2) @ v.abs()).squeeze(-2)
    return ref, bound


def softmax_rows_ref_bound(s, scale):
    """float64 softmax(scale s) of fp32 scores [rows, cols] and the bound of an fp32 implementation: the argument scale s - max carries three
    fp32 roundings of values up to |scale s| + |max| (D = 3 u 2 max|scale s|), exp2 two ulps, the sum (cols + 2) u, the division one:
        |dp| <= (e^(2 D) - 1 + (cols + 6) u) p"""
    s = s.double() * scale
    p = torch.softmax(s, -1)
    D = 6 * U32 * s.abs().amax(-1, keepdim=True)
    return p, (torch.expm1(2 * D) + (s.shape[-1] + 6) * U32) * p


def pixel_locator(N, H, W, C, bq=None, bp=None):
    """flat index of an NHWC [N, H, W, C] tensor -> "(n, y, x, c) [pixel tile, channel tile]" for check_elem's messages"""
    def loc(i):
        p, c = divmod(i, C)
        n, r = divmod(p, H * W)
        y, x = divmod(r, W)
        tile = " pixel %d = tile %d of %d, channel tile %d of %d" % (p, p // bp, bp, c // bq, bq) if bq and bp else " pixel %d" % p
        return "(n, y, x, c) = (%d, %d, %d, %d)%s" % (n, y, x, c, tile)
    return loc
