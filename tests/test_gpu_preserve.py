"""Keeping the unmasked region (`preserve_unmasked`) on the device: the four new kernels through the C ABI (ladi_op_mask_pool8,
ladi_op_mask_feather, ladi_op_image_composite, ladi_op_sched_run_keep) between poisoned rows against tests/preserve_ref.py, then the tiny model
end to end (fused hipGraph, fused eager, modular) against ref_tryon.tryon_reference for all six schedulers, the bit-level guarantees outside
the mask, degenerate masks, stale state and the interplay with strength, the feature cache and a guidance schedule."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import preserve_ref as R
from tests import ref_tryon as RT
from tests import strength_ref as SR
from tests import util as U

pytestmark = pytest.mark.gpu

# (B, h, w) latent shapes: one block; 351 pixels: hw is odd and a 256-thread block straddles two samples.  Image sizes are 8x those
SHAPES = [(2, 8, 12), (3, 9, 13)]


def _P(g):
    return ctypes.c_void_p(g.ptr)


def _rand_mask(B, H, W, seed, p=0.3):
    """a binarised fp16 mask [B, 1, H, W] of blobs: low-resolution noise, upsampled, thresholded"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((B, 1, H // 4, W // 4), generator=g)
    return (F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) > 1 - p).half()


# ------------------------------------------------------------------------------------------------------------------ 1. mask_pool8
def _pool(lib, mask, invert=0):
    B, _, H, W = mask.shape
    gm = U.guarded(mask.reshape(B * H, W).half())
    go = U.guarded_out(B * (H // 8), W // 8, dtype=torch.float32, any_ld=True)
    rc = lib.ladi_op_mask_pool8(_P(gm), B, H, W, invert, _P(go), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    U.assert_untouched(go, "mask_pool8 out")
    U.assert_untouched(gm, "mask_pool8 mask")
    return go.cpu().view(B, 1, H // 8, W // 8)


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_mask_pool8_is_max_pool2d_exactly(lib, B, h, w):
    H, W = 8 * h, 8 * w
    for seed, p in ((1, 0.3), (2, 0.02), (3, 0.9)):
        mask = (torch.rand((B, 1, H, W), generator=torch.Generator().manual_seed(seed)) < p).half()
        want = F.max_pool2d(mask.float(), 8)
        assert torch.equal(_pool(lib, mask), want)
        assert torch.equal(_pool(lib, mask, 1), 1 - want)


def test_mask_pool8_single_pixels_in_the_corners_of_a_footprint(lib):
    B, h, w = SHAPES[1]
    H, W = 8 * h, 8 * w
    for dy, dx in ((0, 0), (0, 7), (7, 0), (7, 7), (3, 4)):
        mask = torch.zeros((B, 1, H, W), dtype=torch.float16)
        mask[1, 0, 8 * 4 + dy, 8 * 11 + dx] = 1
        got = _pool(lib, mask)
        want = torch.zeros((B, 1, h, w))
        want[1, 0, 4, 11] = 1
        assert torch.equal(got, want), (dy, dx)
        assert torch.equal(_pool(lib, mask, 1), R.keep_mask(mask.float()).float())


def test_mask_pool8_refuses_bad_arguments(lib):
    m = torch.zeros((16, 16), dtype=torch.float16, device=U.dev())
    o = torch.zeros(4, device=U.dev())
    assert lib.ladi_op_mask_pool8(ptr(m), 1, 16, 12, 0, ptr(o), stream_ptr()) < 0 and "multiples of 8" in _lib.last_error()
    assert lib.ladi_op_mask_pool8(None, 1, 16, 16, 0, ptr(o), stream_ptr()) < 0
    assert lib.ladi_op_mask_pool8(ctypes.c_void_p(m.data_ptr() + 2), 1, 8, 8, 0, ptr(o), stream_ptr()) < 0 and "aligned" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------ 2. mask_feather
def _feather(lib, mask, sigma):
    B, _, H, W = mask.shape
    gm = U.guarded(mask.reshape(B * H, W).half(), any_ld=True)
    gt = U.guarded_out(B * H, W, dtype=torch.float32, any_ld=True)
    go = U.guarded_out(B * H, W, dtype=torch.float32, any_ld=True)
    r = lib.ladi_op_mask_feather(_P(gm), B, H, W, sigma, _P(gt), _P(go), stream_ptr())
    assert r >= 0, _lib.last_error()
    torch.cuda.synchronize()
    for g_, what in ((gm, "mask"), (gt, "tmp"), (go, "out")):
        U.assert_untouched(g_, "mask_feather " + what)
    return go.cpu().view(B, 1, H, W), r


@pytest.mark.parametrize("sigma", [0.5, 2.0, 4.0])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_mask_feather_vs_reference(lib, B, h, w, sigma):
    """two passes, each a convex fp32 sum of 2r + 1 values in [0, 1] (error <= (2r + 2) 2^-24 with the products), a factor 2 for the fp32
    weights: |err| <= 4 (2r + 2) 2^-24.  The blobs touch the image border, so the replicate rule is exercised; two calls are bit-equal"""
    H, W = 8 * h, 8 * w
    mask = _rand_mask(B, H, W, 11 + h)
    mask[:, :, :, :3] = 1            # a mask edge 3 pixels from the left border, and one on the bottom border
    mask[:, :, H - 2:, :] = 1
    mask[0, :, :5, W - 4:] = 1
    got, r = _feather(lib, mask, sigma)
    ref = R.feather(mask.float(), sigma)
    _, r_ref = R.feather_weights(sigma)
    assert r == r_ref
    bound = 4 * (2 * r + 2) * 2.0 ** -24
    err = float((got.double() - ref).abs().max())
    print("mask_feather B=%d %dx%d sigma=%.1f r=%d: max abs err %.3g (bound %.3g)" % (B, H, W, sigma, r, err, bound))
    assert torch.isfinite(got).all() and err <= bound, (err, bound)
    got2, _ = _feather(lib, mask, sigma)
    assert torch.equal(got, got2)


@pytest.mark.parametrize("sigma", [0.5, 4.0])
def test_mask_feather_keeps_constant_masks_exactly(lib, sigma):
    B, h, w = SHAPES[0]
    for v in (0.0, 1.0):
        mask = torch.full((B, 1, 8 * h, 8 * w), v, dtype=torch.float16)
        got, _ = _feather(lib, mask, sigma)
        assert (got == v).all()


def test_mask_feather_far_from_an_edge_is_exact(lib):
    """more than r pixels inside a region the mask is constant over every tap: the composite's select relies on exact 0 there"""
    B, H, W = 1, 64, 96
    mask = torch.zeros((B, 1, H, W), dtype=torch.float16)
    mask[:, :, :, 48:] = 1
    got, r = _feather(lib, mask, 2.0)
    assert r == 6 and (got[..., :48 - r] == 0).all() and (got[..., 48 + r:] == 1).all()
    edge = got[..., 48 - r:48 + r]
    assert float(edge.min()) > 0 and float(edge.max()) < 1


def test_mask_feather_refuses_bad_arguments(lib):
    m = torch.zeros((8, 8), dtype=torch.float16, device=U.dev())
    a, b = torch.zeros((8, 8), device=U.dev()), torch.zeros((8, 8), device=U.dev())
    for s in (0.0, -1.0, 32.5, float("nan")):
        assert lib.ladi_op_mask_feather(ptr(m), 1, 8, 8, s, ptr(a), ptr(b), stream_ptr()) < 0 and "sigma" in _lib.last_error(), s
    assert lib.ladi_op_mask_feather(ptr(m), 1, 8, 8, 1.0, ptr(a), ptr(a), stream_ptr()) < 0
    assert lib.ladi_op_mask_feather(ptr(m), 1, 8, 8, 32.0, ptr(a), ptr(b), stream_ptr()) == 96, _lib.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 3. image_composite
def _nhwc8(x):
    """NCHW [B, 3, H, W] -> fp16 rows [B H W, 4] (a fourth lane of junk the kernels never use)"""
    B, _, H, W = x.shape
    rows = torch.full((B * H * W, 4), 0.37, dtype=torch.float16)
    rows[:, :3] = x.permute(0, 2, 3, 1).reshape(-1, 3).half()
    return rows


def _u8_out(n):
    """a uint8 output of n bytes 32 bytes into an allocation of 0xA5 bytes"""
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=U.dev())
    return buf, ctypes.c_void_p(buf.data_ptr() + 32)


def _u8_check(buf, n):
    b = buf.cpu()
    assert (b[:32] == 0xA5).all() and (b[32 + n:] == 0xA5).all(), "u8 output: bytes around it were overwritten"
    return b[32:32 + n]


def _image_post(lib, rows, u8):
    n = rows.shape[0]
    gs = U.guarded(rows, ld=8)
    if u8:
        buf, p = _u8_out(n * 3)
        assert lib.ladi_op_image_post(_P(gs), 8, n, p, 1, stream_ptr()) == 0
        torch.cuda.synchronize()
        return _u8_check(buf, n * 3).view(n, 3)
    go = U.guarded_out(n, 3, dtype=torch.float32, any_ld=True)
    assert lib.ladi_op_image_post(_P(gs), 8, n, _P(go), 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    return go.cpu()


def _composite(lib, decoded_rows, image, mask, u8):
    """decoded_rows fp16 [B HW, 4] at ld = 8; image NCHW fp16 / fp32; mask [B, 1, H, W] fp16 (binary) or fp32"""
    B, _, H, W = image.shape
    n = B * H * W
    gs = U.guarded(decoded_rows, ld=8)
    gi = U.guarded(image.reshape(B * 3 * H, W).contiguous(), any_ld=True)
    gm = U.guarded(mask.reshape(B * H, W).contiguous(), any_ld=True)
    args = (_P(gs), 8, _P(gi), 0 if image.dtype == torch.float32 else 1, _P(gm), 1 if mask.dtype == torch.float32 else 0, B, H * W)
    if u8:
        buf, p = _u8_out(n * 3)
        rc = lib.ladi_op_image_composite(*args, p, 1, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        out = _u8_check(buf, n * 3).view(n, 3)
    else:
        go = U.guarded_out(n, 3, dtype=torch.float32, any_ld=True)
        rc = lib.ladi_op_image_composite(*args, _P(go), 0, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        U.assert_untouched(go, "image_composite out")
        out = go.cpu()
    for g_, what in ((gs, "decoded"), (gi, "image"), (gm, "mask")):
        U.assert_untouched(g_, "image_composite " + what)
    return out


def _composite_case(B, h, w, dtype, seed):
    H, W = 8 * h, 8 * w
    g = torch.Generator().manual_seed(seed)
    decoded = (torch.rand((B, 3, H, W), generator=g) * 2.6 - 1.3).half()        # some of it clamps at both ends
    image = (torch.rand((B, 3, H, W), generator=g) * 2 - 1).half().to(dtype)    # fp16-representable: image_post can be handed the same values
    mask = _rand_mask(B, H, W, seed + 1, p=0.5)
    return decoded, image, mask


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_image_composite_binary_mask_selects_bitwise(lib, B, h, w, dtype, u8):
    """M = 0: image_post of the input image; M = 1: image_post of the decoded tensor; a NaN in the decoded tensor under M = 0 stays out"""
    decoded, image, mask = _composite_case(B, h, w, dtype, 41)
    m = mask.reshape(-1) > 0.5
    rows = _nhwc8(decoded.float())
    want_g, want_p = _image_post(lib, rows, u8), _image_post(lib, _nhwc8(image.float()), u8)
    rows_nan = rows.clone()
    rows_nan[~m, :3] = float("nan")
    got = _composite(lib, rows_nan, image, mask, u8)
    assert m.any() and (~m).any()
    assert torch.equal(got[m], want_g[m]) and torch.equal(got[~m], want_p[~m])
    if not u8:
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_image_composite_feathered_mask_vs_reference(lib, B, h, w, dtype):
    """fp32: M g + (1 - M) p within 2^-22 of float64 (g, p, 1 - M, two products and a sum, each rounded once on values <= 1); u8: at most 1 off,
    and equal wherever 255 v is farther than 1e-3 from a rounding boundary (fewer than 1 % of the pixels are that close)"""
    decoded, image, mask = _composite_case(B, h, w, dtype, 43)
    H, W = 8 * h, 8 * w
    soft = R.feather(mask.float(), 2.0).float()
    assert ((soft > 0) & (soft < 1)).any() and (soft == 0).any()
    rows = _nhwc8(decoded.float())
    ref = R.composite(decoded.float(), image.float(), soft).reshape(-1, 3)
    got = _composite(lib, rows, image, soft, False)
    err = float((got.double() - ref).abs().max())
    got8 = _composite(lib, rows, image, soft, True)
    v = ref * 255
    d8 = (got8.double() - v.round()).abs()
    far = ((v - v.floor()) - 0.5).abs() > 1e-3
    share = 1 - float(far.double().mean())
    print("image_composite %s B=%d %dx%d: fp32 max abs err %.3g (bound %.3g); u8 max diff %d, %.3f %% within 1e-3 of a boundary"
          % (str(dtype).split(".")[-1], B, H, W, err, 2.0 ** -22, int(d8.max()), 100 * share))
    assert err <= 2.0 ** -22, err
    assert int(d8.max()) <= 1 and (d8[far] == 0).all()
    assert share < 0.01, share


def test_image_composite_unaligned_pointers_take_the_element_path(lib):
    """pointers 4 bytes off the vector alignment give the same bits"""
    B, h, w = SHAPES[0]
    decoded, image, mask = _composite_case(B, h, w, torch.float32, 47)
    H, W = 8 * h, 8 * w
    n = B * H * W
    soft = R.feather(mask.float(), 2.0).float()
    rows = _nhwc8(decoded.float())
    want = _composite(lib, rows, image, soft, False)
    d = U.dev()
    src = torch.zeros((n, 8), dtype=torch.float16, device=d)
    src[:, :4] = rows.to(d)
    img = torch.zeros(image.numel() + 1, device=d)
    img[1:] = image.reshape(-1).to(d)
    msk = torch.zeros(n + 1, device=d)
    msk[1:] = soft.reshape(-1).to(d)
    out = torch.full((n * 3 + 2,), -3.0, device=d)
    rc = lib.ladi_op_image_composite(ptr(src), 8, ctypes.c_void_p(img.data_ptr() + 4), 0, ctypes.c_void_p(msk.data_ptr() + 4), 1, B, H * W,
                                     ctypes.c_void_p(out.data_ptr() + 4), 0, stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    o = out.cpu()
    assert o[0] == -3.0 and o[-1] == -3.0 and torch.equal(o[1:-1].view(n, 3), want)


def test_image_composite_refuses_bad_arguments(lib):
    d = U.dev()
    s, i, m, o = (torch.zeros((16, 8), dtype=torch.float16, device=d), torch.zeros((1, 3, 4, 4), device=d), torch.zeros((16,), device=d),
                  torch.zeros((16, 3), device=d))
    f = lib.ladi_op_image_composite
    assert f(ptr(s), 8, ptr(i), 0, ptr(m), 1, 1, 16, ptr(o), 0, stream_ptr()) == 0, _lib.last_error()
    assert f(ptr(s), 8, ptr(i), 0, ptr(m), 1, 1, 14, ptr(o), 0, stream_ptr()) < 0 and "multiple of 4" in _lib.last_error()
    assert f(ptr(s), 6, ptr(i), 0, ptr(m), 1, 1, 16, ptr(o), 0, stream_ptr()) < 0 and "ld" in _lib.last_error()
    assert f(ptr(s), 8, ptr(i), 7, ptr(m), 1, 1, 16, ptr(o), 0, stream_ptr()) < 0 and "dtype" in _lib.last_error()
    assert f(None, 8, ptr(i), 0, ptr(m), 1, 1, 16, ptr(o), 0, stream_ptr()) < 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 4. sched_run_keep
def _keep_case(kind, B, h, w, seed=71, all_ones=False):
    sch = SR.make_mirror(kind)
    steps = 8
    sch.set_timesteps(steps)
    n = len(sch.timesteps)                                   # PNDM: 9, with its repeated timestep
    table = ([7.5, 3.0, 1.0, 0.5, 9.0, 1.0, 0.0, 5.0] + [2.0] * n)[:n]
    hw = h * w
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((n, 2 * B, hw, 4), generator=g).half()
    lat0 = torch.randn((B, 4, h, w), generator=g) * sch.init_noise_sigma
    z0 = torch.randn((B, 4, h, w), generator=g)
    z0[0, 0, 0, 0], z0[0, 1, 0, 0] = -0.0, 1e-42             # a negative zero and a subnormal at a keep pixel survive
    noise = torch.randn((B, 4, h, w), generator=g)
    step_noise = torch.stack([torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(17 + i)) for i in range(n)])
    if all_ones:
        mask = torch.ones((B, 1, 8 * h, 8 * w))
    else:
        # about half of the latent pixels have their whole footprint unmasked; the others hold between one and 64 masked pixels
        full = (torch.rand((B, 1, h, w), generator=g) < 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        mask = full * (torch.rand((B, 1, 8 * h, 8 * w), generator=g) < 0.2).float()
        mask[:, :, ::8, ::8] = full[:, :, ::8, ::8].clone() * mask[:, :, 7::8, 7::8]       # the top-left sample alone would often say "unmasked"
        mask = torch.maximum(mask, full * F.one_hot(torch.randint(0, 64, (B, 1, h, w), generator=g), 64).view(B, 1, h, w, 8, 8)
                             .permute(0, 1, 2, 4, 3, 5).reshape(B, 1, 8 * h, 8 * w).float())
        mask[0, 0, :8, :8] = 0                               # latent pixel (0, 0) of sample 0 is a keep pixel
    return sch, steps, n, table, eps, lat0, z0, noise, step_noise, R.keep_mask(mask)


def _pix(t):
    B = t.shape[0]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _run_keep(lib, sch, steps, n, table, eps, B, hw, lat0, step_noise, keep=None, z0=None, noise=None):
    L_ = _pix(lat0).to(U.dev())
    N = step_noise.contiguous().to(U.dev())
    E = eps.to(U.dev())
    ac = P.alphas_cumprod().contiguous()
    tab = (ctypes.c_float * n)(*table)
    if keep is None:
        rc = lib.ladi_op_sched_run_guided(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, ptr(E), 4, n, B, hw, tab, 0.0, ptr(L_), ptr(N), n,
                                          stream_ptr())
    else:
        gz, gn = U.guarded(_pix(z0)), U.guarded(_pix(noise))
        gk = U.guarded(_pix(keep.float()), any_ld=True)
        rc = lib.ladi_op_sched_run_keep(sch.kind, steps, ctypes.c_void_p(ac.data_ptr()), 0.0, ptr(E), 4, n, B, hw, tab, 0.0, ptr(L_), ptr(N), n,
                                        _P(gz), _P(gn), _P(gk), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    if keep is not None:
        for g_, what in ((gz, "z0"), (gn, "noise"), (gk, "mask")):
            U.assert_untouched(g_, "sched_run_keep " + what)
    return L_.cpu()


@pytest.mark.parametrize("B,h,w", SHAPES)
@pytest.mark.parametrize("kind", R.SCHEDULERS)
def test_sched_run_keep_vs_reference(lib, kind, B, h, w, monkeypatch):
    """the step kernel with the blend over a random eps sequence and a guidance table with cond-only evaluations against the float64 loop of
    preserve_ref: rel-L2 < 1e-5 (the bound of test_sched_run_guided_vs_reference for this arithmetic); keep pixels end as z0 bit for bit; NaN
    in eps at keep pixels changes nothing"""
    import ladi_vton_amd.schedulers as S
    sch, steps, n, table, eps, lat0, z0, noise, step_noise, keep = _keep_case(kind, B, h, w)
    hw = h * w
    draws = iter(step_noise)
    monkeypatch.setattr(S, "_step_noise", lambda shape, dtype, generator, device: next(draws).to(dtype))
    e_nchw = eps.view(n, 2 * B, h, w, 4).permute(0, 1, 4, 2, 3)
    ref = R.sched_reference(sch, e_nchw, table, 0.0, lat0, keep, z0, noise)
    got_pix = _run_keep(lib, sch, steps, n, table, eps, B, hw, lat0, step_noise, keep, z0, noise)
    got = got_pix.view(B, h, w, 4).permute(0, 3, 1, 2)
    err = U.rel_l2(got, ref)
    k4 = keep.expand(B, 4, h, w)
    print("sched_run_keep %s B=%d hw=%d: rel-L2 %.3g, %d of %d pixels kept" % (kind, B, hw, err, int(keep.sum()), B * hw))
    assert keep.any() and (~keep).any()
    assert torch.isfinite(got).all() and err < 1e-5, err
    assert torch.equal(got[k4].view(torch.int32), z0[k4].view(torch.int32))
    assert not torch.equal(got[~k4], z0[~k4])
    eps_nan = eps.clone().view(n, 2, B, h, w, 4)
    eps_nan[:, :, keep[:, 0]] = float("nan")
    got_nan = _run_keep(lib, sch, steps, n, table, eps_nan.view(n, 2 * B, hw, 4), B, hw, lat0, step_noise, keep, z0, noise)
    assert torch.equal(got_nan, got_pix)


@pytest.mark.parametrize("kind", R.SCHEDULERS)
def test_sched_run_keep_with_nothing_to_keep_is_the_guided_run_bitwise(lib, kind):
    B, h, w = SHAPES[1]
    sch, steps, n, table, eps, lat0, z0, noise, step_noise, keep = _keep_case(kind, B, h, w, all_ones=True)
    assert not keep.any()
    a = _run_keep(lib, sch, steps, n, table, eps, B, h * w, lat0, step_noise, keep, z0, noise)
    b = _run_keep(lib, sch, steps, n, table, eps, B, h * w, lat0, step_noise)
    assert torch.equal(a, b)


def test_sched_run_keep_refuses_null_buffers(lib):
    B, h, w = SHAPES[0]
    sch, steps, n, table, eps, lat0, z0, noise, step_noise, keep = _keep_case("ddim", B, h, w)
    d = U.dev()
    L_, E, Z, K = _pix(lat0).to(d), eps.to(d), _pix(z0).to(d), _pix(keep.float()).to(d)
    tab = (ctypes.c_float * n)(*table)
    f = lib.ladi_op_sched_run_keep
    assert f(0, steps, None, 0.0, ptr(E), 4, n, B, h * w, tab, 0.0, ptr(L_), None, 0, None, ptr(Z), ptr(K), stream_ptr()) < 0 and "null" in _lib.last_error()
    assert f(0, steps, None, 0.0, ptr(E), 4, n, B, h * w, tab, 0.0, ptr(L_), None, 0, ptr(Z), ptr(Z), None, stream_ptr()) < 0
    assert f(0, steps, None, 0.0, ptr(E), 4, n, B, h * w, tab, 0.0, ptr(L_), None, 0, ctypes.c_void_p(Z.data_ptr() + 4), ptr(Z), ptr(K),
             stream_ptr()) < 0 and "aligned" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, inp={})


STEPS = 8
B_, H_, W_ = 2, 256, 192
ARMS = {"graph": (True, True), "eager": (True, False), "modular": (False, False)}
NOISE_SEED = 5


def _ragged_mask():
    """a region whose edge is aligned to 8 nowhere: rows 61 .. 202, every row's ends moving with y"""
    m = torch.zeros((B_, 1, H_, W_))
    for y in range(61, 203):
        m[:, 0, y, 45 + y % 7:150 - y % 5] = 1.0
    m[1, 0, 20:27, 11:19] = 1.0          # a second, small island in sample 1
    return m


def _inputs(tiny, mask="ragged"):
    if mask not in tiny["inp"]:
        inp = dict(P.synthetic_inputs(B_, H_, W_, L=8, D=tiny["ucfg"]["cross_attention_dim"]))
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        inp["mask_image"] = {"ragged": _ragged_mask, "ones": lambda: torch.ones((B_, 1, H_, W_)), "zeros": lambda: torch.zeros((B_, 1, H_, W_))}[mask]()
        tiny["inp"][mask] = inp
    return tiny["inp"][mask]


def _pipe(tiny, sched):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=SR.make_mirror(sched), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, fused=True, graph=True, mask="ragged", prompt=None, **kw):
    """-> (images, latents)"""
    inp = _inputs(tiny, mask)
    d = U.dev()
    kw.setdefault("generator", torch.Generator().manual_seed(NOISE_SEED))
    pe = inp["prompt_embeds"] if prompt is None else prompt
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=pe.to(d), negative_prompt_embeds=inp["negative_prompt_embeds"].to(d),
               height=H_, width=W_, num_inference_steps=STEPS, output_type="np", fused=fused, use_graph=graph,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _ref(tiny, sched, key, mode="both", mask="ragged", feather_sigma=0.0, interval=None, **kw):
    key = (sched, key)
    if key not in tiny["ref"]:
        sd = tiny["sd"]
        tiny["ref"][key] = RT.tryon_reference(sd["unet"], tiny["ucfg"], sd["vae"], tiny["vcfg"], sd["emasc"], _inputs(tiny, mask), STEPS, sched,
                                              preserve=(mode, feather_sigma), feature_cache=(interval, 0),
                                              generator=torch.Generator().manual_seed(NOISE_SEED), **kw)
    return tiny["ref"][key]


def _run(tiny, sched, arm, mask="ragged"):
    """one run per (scheduler, arm, mask) on a fresh pipeline: "plain" is the fused hipGraph run without the feature, the others run "both\""""
    key = (sched, arm, mask)
    if key not in tiny["run"]:
        kw = {} if arm == "plain" else dict(preserve_unmasked="both")
        tiny["run"][key] = _call(tiny, _pipe(tiny, sched), *ARMS["graph" if arm == "plain" else arm], mask=mask, **kw)
    return tiny["run"][key]


def _keep(tiny, mask="ragged"):
    return R.keep_mask(_inputs(tiny, mask)["mask_image"])           # bool [B, 1, h, w]


def _z0(tiny, mask="ragged"):
    """scaling * mode(pipe.vae.encode(image)) with the pipeline's own VAE"""
    image = _inputs(tiny, mask)["image"].to(U.dev())
    mode = tiny["mod"]["vae"].encode(image)[0].latent_dist.mode()
    return (tiny["vcfg"]["scaling_factor"] * mode.float()).cpu()


def _post(image):
    """clamp(image / 2 + 0.5, 0, 1) in fp32, NHWC: x / 2 is exact, so the one rounding is the same on every device"""
    return (image.float() * 0.5 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).contiguous()


# --- 5
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("sched", R.SCHEDULERS)
def test_tryon_tiny_both_vs_reference(tiny, sched, arm):
    """B = 2, 256x192, 8 steps, a ragged mask, "both": fused hipGraph, fused eager and modular against ref_tryon.tryon_reference; the
    thresholds tests/test_gpu_strength.py applies to the same arms (latents >= 40 dB, image >= 35 dB on [0, 1])"""
    ref_img, ref_lat = _ref(tiny, sched, "both")
    img, lat = _run(tiny, sched, arm)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny preserve both %s %s: image %.2f dB, latents %.2f dB" % (sched, arm, p_img, p_lat))
    assert img.shape == ref_img.shape and torch.isfinite(lat).all()
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


@pytest.mark.parametrize("sched", R.SCHEDULERS)
def test_tryon_tiny_both_graph_equals_eager_bitwise(tiny, sched):
    img_g, lat_g = _run(tiny, sched, "graph")
    img_e, lat_e = _run(tiny, sched, "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)
    # and it is not the plain run: the comparisons see the feature
    img_p, lat_p = _run(tiny, sched, "plain")
    assert not torch.equal(lat_p, lat_g) and not torch.equal(img_p, img_g)


def test_tryon_tiny_feathered_both_vs_reference(tiny):
    ref_img, ref_lat = _ref(tiny, "ddim", "feather", feather_sigma=2.0)
    img, lat = _call(tiny, _pipe(tiny, "ddim"), preserve_unmasked="both", mask_feather=2.0)
    img_m, lat_m = _call(tiny, _pipe(tiny, "ddim"), False, False, preserve_unmasked="both", mask_feather=2.0)
    p_img, p_lat, p_mod = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat), U.psnr(img_m, ref_img, peak=1.0)
    print("tiny preserve both, feather 2: image %.2f dB (modular %.2f dB), latents %.2f dB" % (p_img, p_mod, p_lat))
    assert p_lat >= 40.0 and p_img >= 35.0 and p_mod >= 35.0
    assert not torch.equal(img, _run(tiny, "ddim", "graph")[0])


# --- 6
def test_pixels_mode_is_bit_exact_on_both_sides_of_the_mask(tiny):
    """"pixels", no feather: outside the mask the input image's post-processed values, inside the plain run's, bit for bit, in fp32 and uint8;
    the latents are the plain run's"""
    inp = _inputs(tiny)
    img_p, lat_p = _run(tiny, "ddim", "plain")
    pipe = _pipe(tiny, "ddim")
    img, lat = _call(tiny, pipe, preserve_unmasked="pixels")
    m = (inp["mask_image"] >= 0.5)[:, 0]                     # [B, H, W]
    want_out = _post(inp["image"])
    assert torch.equal(lat, lat_p)
    assert torch.equal(img[~m], want_out[~m]) and torch.equal(img[m], img_p[m])
    assert not torch.equal(img, img_p)
    # uint8 (ladi_tryon_run_u8): the same select on round(255 v)
    d = U.dev()
    args = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
            inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H_, W_, STEPS, 7.5, 1.0, False, True)
    u8 = pipe._run_fused(*args, return_device=True, out_uint8=True, preserve=(2, 0.0)).cpu()
    u8_plain = pipe._run_fused(*args, return_device=True, out_uint8=True).cpu()
    assert not pipe.check_overflow()
    want8 = (want_out * 255).round().to(torch.uint8)
    assert u8.dtype == torch.uint8 and torch.equal(u8[~m], want8[~m]) and torch.equal(u8[m], u8_plain[m])
    assert torch.equal(u8_plain, (img_p * 255).round().to(torch.uint8))


# --- 7
def test_latents_mode_keeps_the_keep_pixels_whatever_the_prompt(tiny):
    """two runs with different prompt_embeds: last_latents at keep pixels bit-equal across them and equal to scaling * mode(vae.encode(image)),
    bit for bit (the bound the strength tests use for init_image: the same encode gives the same bits); inside the mask they differ"""
    inp = _inputs(tiny)
    pipe = _pipe(tiny, "ddim")
    other = torch.randn(inp["prompt_embeds"].shape, generator=torch.Generator().manual_seed(99)).half().float()
    _, lat_a = _call(tiny, pipe, preserve_unmasked="latents")
    _, lat_b = _call(tiny, pipe, preserve_unmasked="latents", prompt=other)
    k4 = _keep(tiny).expand(B_, 4, H_ // 8, W_ // 8)
    z0 = _z0(tiny)
    print("latents mode: %d of %d latent pixels kept; max |latents - z0| at keep pixels %.3g"
          % (int(_keep(tiny).sum()), B_ * (H_ // 8) * (W_ // 8), float((lat_a[k4] - z0[k4]).abs().max())))
    assert k4.any() and (~k4).any()
    assert torch.equal(lat_a[k4], lat_b[k4]) and not torch.equal(lat_a[~k4], lat_b[~k4])
    assert torch.equal(lat_a[k4], z0[k4])


@pytest.mark.parametrize("arm", ["graph", "modular"])
@pytest.mark.parametrize("sched", ["ddim", "pndm", "euler_a"])
def test_step_callback_sees_the_blended_latents(tiny, sched, arm):
    """after evaluation i the keep pixels hold k_x[i] z0 + k_n[i] noise: rel-L2 < 1e-5 (fp32 arithmetic on fp32 coefficients)"""
    seen = []
    pipe = _pipe(tiny, sched)
    _call(tiny, pipe, *ARMS[arm], preserve_unmasked="latents", callback=lambda i, t, x: seen.append(x.detach().float().cpu().clone()))
    s = SR.make_mirror(sched)
    s.set_timesteps(STEPS)
    kc = R.keep_coeffs(s)
    assert len(seen) == len(kc)
    k4 = _keep(tiny).expand(B_, 4, H_ // 8, W_ // 8)
    z0, noise = _z0(tiny).double(), _inputs(tiny)["noise_latents"].double()
    worst = 0.0
    for i, x in enumerate(seen):
        want = kc[i][0] * z0 + kc[i][1] * noise
        worst = max(worst, U.rel_l2(x[k4], want[k4]))
    print("callback %s %s: worst rel-L2 at keep pixels %.3g" % (sched, arm, worst))
    assert worst < 1e-5, worst


# --- 8
def test_all_ones_mask_is_the_plain_run_bitwise(tiny):
    img_p, lat_p = _run(tiny, "ddim", "plain", mask="ones")
    img, lat = _run(tiny, "ddim", "graph", mask="ones")
    assert torch.equal(lat, lat_p) and torch.equal(img, img_p)


def test_all_zeros_mask_returns_the_input(tiny):
    img, lat = _run(tiny, "ddim", "graph", mask="zeros")
    assert torch.equal(img, _post(_inputs(tiny, "zeros")["image"]))
    assert torch.equal(lat, _z0(tiny, "zeros"))


# --- 9
@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_nothing_stale_survives_a_preserve_run(tiny, sched):
    """a handle that ran "both" and then runs plain equals a fresh handle's plain run bit for bit, and the other way round"""
    img_b, lat_b = _run(tiny, sched, "graph")
    img_p, lat_p = _run(tiny, sched, "plain")
    pipe = _pipe(tiny, sched)
    _, lat_1 = _call(tiny, pipe, preserve_unmasked="both")
    img_2, lat_2 = _call(tiny, pipe)
    img_3, lat_3 = _call(tiny, pipe, preserve_unmasked="both")
    assert torch.equal(lat_1, lat_b)
    assert torch.equal(lat_2, lat_p) and torch.equal(img_2, img_p)
    assert torch.equal(lat_3, lat_b) and torch.equal(img_3, img_b)


def test_both_with_strength(tiny):
    init = SR.synthetic_init(B_, H_ // 8, W_ // 8)
    ref_img, ref_lat = _ref(tiny, "ddim", "strength", init_latents=init, first_step=4)
    img, lat = _call(tiny, _pipe(tiny, "ddim"), preserve_unmasked="both", strength=0.5, init_latents=init)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny preserve both + strength 0.5: image %.2f dB, latents %.2f dB" % (p_img, p_lat))
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)
    k4 = _keep(tiny).expand(B_, 4, H_ // 8, W_ // 8)
    assert torch.equal(lat[k4], _z0(tiny)[k4])


def test_both_with_feature_cache(tiny):
    ref_img, ref_lat = _ref(tiny, "ddim", "cache", interval=2)
    pipe = _pipe(tiny, "ddim")
    img, lat = _call(tiny, pipe, preserve_unmasked="both", feature_cache=2)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny preserve both + feature_cache 2: image %.2f dB, latents %.2f dB" % (p_img, p_lat))
    assert pipe.shallow_evals == 4
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


def test_both_with_a_guidance_schedule(tiny):
    import ladi_vton_amd as L
    table = L.guidance_interval(STEPS, 7.5, 0.0, 0.5)              # CFG on the first half, cond-only after
    ref_img, ref_lat = _ref(tiny, "ddim", "schedule", table=table)
    pipe = _pipe(tiny, "ddim")
    img, lat = _call(tiny, pipe, preserve_unmasked="both", guidance_scale=table)
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("tiny preserve both + guidance schedule: image %.2f dB, latents %.2f dB" % (p_img, p_lat))
    assert pipe.cond_only_evals() == 4
    assert p_lat >= 40.0 and p_img >= 35.0, (p_img, p_lat)


def test_setter_refusals_leave_the_handle_usable(tiny, lib):
    pipe = _pipe(tiny, "ddim")
    _, lat = _call(tiny, pipe, preserve_unmasked="both")
    h = pipe._tryon
    assert lib.ladi_tryon_set_preserve(h, 4, 0.0) < 0 and "mode bits" in _lib.last_error()
    assert lib.ladi_tryon_set_preserve(h, 1, 1.0) < 0 and "pixels" in _lib.last_error()
    assert lib.ladi_tryon_set_preserve(h, 2, 33.0) < 0
    assert lib.ladi_tryon_set_preserve(h, 3, 32.0) == 0 and lib.ladi_tryon_set_preserve(h, 0, 0.0) == 0
    _, lat_2 = _call(tiny, pipe, preserve_unmasked="both")
    assert torch.equal(lat_2, lat) and torch.equal(lat, _run(tiny, "ddim", "graph")[1])
