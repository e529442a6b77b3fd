"""Image sizes divisible by 8 whose latent is not a multiple of 8 (640x480, 136x120, ...): the size-mapped nearest upsample folded into the
implicit-GEMM gather and stride-2 convolutions on odd sides, both through the C ABI (ladi_op_igemm); the UNet forward of the tiny and the
full-size model against tests/ref_unet.py (diffusers' `forward_upsample_size` arithmetic); the fused and modular try-on loops of the tiny
model against the oracle pipeline running that forward."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P
from tests import ref_unet as R
from tests import util as U

pytestmark = pytest.mark.gpu
TOL = 2e-3


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


def _conv(x, wt, cout, Ho, Wo, stride=1, pad=1, ups=0, x2=None, bias=None, cfg=0):
    """one ladi_op_igemm launch with an explicit output size (tests/util.py's helper derives it from the 2x rule); returns (rc, NCHW out)"""
    lib = _lib.load()
    xs = U.nhwc16(x)
    x2s = U.nhwc16(x2) if x2 is not None else None
    N, H, W, C0 = xs.shape
    C1 = x2s.shape[3] if x2s is not None else 0
    wp = U.pack_conv_weight(wt)
    out = torch.zeros((N, Ho, Wo, cout), dtype=torch.float16, device=U.dev())
    d = U.IGemmDesc()
    d.src0, d.C0, d.ld0 = xs.data_ptr(), C0, C0
    if x2s is not None:
        d.src1, d.C1, d.ld1 = x2s.data_ptr(), C1, C1
    d.Hs, d.Ws, d.Ho, d.Wo, d.P = H, W, Ho, Wo, N * Ho * Wo
    d.ksize, d.stride, d.pad, d.ups = wt.shape[-1], stride, pad, ups
    d.W, d.Q, d.K, d.ldw = wp.data_ptr(), cout, wt.shape[-1] ** 2 * (C0 + C1), 0
    b = None
    if bias is not None:
        b = bias.half().to(U.dev())
        d.bias = b.data_ptr()
    d.act, d.out_scale = 0, 1.0
    d.out, d.ldo = out.data_ptr(), cout
    rc = lib.ladi_op_igemm(ctypes.byref(d), 1, cfg, stream_ptr())
    torch.cuda.synchronize()
    return rc, U.to_nchw(out)


CFGS = [0, 3, 7, 32, 33, 47]     # tuner's choice, ring-staged tiles, the staggered large-tile kernel


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("hw", [(15, 9), (7, 5), (30, 15)])
def test_stride2_conv_on_odd_sides(cfg, hw):
    """the UNet's downsampler (k3, s2, p1) on odd sides gives ceil(H / 2) rows, as torch does.  Ho / Wo are passed explicitly, so this
    covers the kernels (which handled it before); the host-side sizing in conv2d is guarded by the UNet forward tests below"""
    h, w = hw
    x, wt, b = _rand((2, 128, h, w), 1), _rand((192, 128, 3, 3), 2, 0.03), _rand((192,), 3, 0.1)
    Ho, Wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rc, y = _conv(x, wt, 192, Ho, Wo, stride=2, bias=b, cfg=cfg)
    assert rc == 0, (rc, _lib.last_error())
    ref = F.conv2d(x, wt, b, stride=2, padding=1)
    assert y.shape == ref.shape and U.rel_l2(y, ref) < TOL


UPS = [((3, 8), (5, 15)), ((9, 3), (17, 5)), ((8, 9), (15, 17)), ((10, 7), (20, 15)), ((5, 4), (9, 7)), ((6, 4), (12, 8))]   # last: 2x control


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("src,dst", UPS)
def test_size_mapped_upsample_conv(src, dst, two, cfg):
    """nearest upsample to an arbitrary size folded into the 3x3 gather == F.interpolate(size=...) then F.conv2d, one or two sources"""
    (h, w), (Ho, Wo) = src, dst
    x = _rand((2, 128, h, w), 10)
    x2 = _rand((2, 64, h, w), 11) if two else None
    cin = 128 + (64 if two else 0)
    wt, b = _rand((160, cin, 3, 3), 12, 0.03), _rand((160,), 13, 0.1)
    rc, y = _conv(x, wt, 160, Ho, Wo, ups=1, x2=x2, bias=b, cfg=cfg)
    assert rc == 0, (rc, _lib.last_error())
    xin = torch.cat([x, x2], 1) if two else x
    ref = F.conv2d(F.interpolate(xin, size=(Ho, Wo), mode="nearest"), wt, b, padding=1)
    assert U.rel_l2(y, ref) < TOL, U.rel_l2(y, ref)


@pytest.mark.parametrize("cfg", [104, 105, 106])
def test_halo_upsample_forms_refuse_non_2x(cfg):
    """the folded-upsample halo forms know only nearest-2x: a size-mapped descriptor is refused, not mis-computed"""
    wt = _rand((128, 128, 3, 3), 21, 0.03)
    rc, _ = _conv(_rand((1, 128, 9, 12), 20), wt, 128, 16, 24, ups=1, cfg=cfg)     # 9 -> 16 rows: whole tiles, but not a doubling
    assert rc != 0
    x = _rand((1, 128, 8, 12), 22)
    rc, y = _conv(x, wt, 128, 16, 24, ups=1, cfg=cfg)          # the 2x control still runs there
    assert rc == 0 and U.rel_l2(y, F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, padding=1)) < TOL


@pytest.mark.parametrize("hd,T", [(512, 255), (512, 2701), (128, 375), (128, 17), (256, 1)])
def test_flash_attention_wide_ragged_tokens(lib, hd, T):
    """the VAE mid-block attention at token counts that are not a multiple of 4 (latents 17x15, 15x25, ...): V^T rows padded to a multiple
    of 4, the last partial 4-key segment read element by element; vs torch softmax(QK^T / sqrt(d)) V in fp32 (tolerance of test_gpu_ops)"""
    n, ldv = 2, (T + 3) // 4 * 4
    q, k, v = _rand((n, T, hd), 95), _rand((n, T, hd), 96), _rand((n, T, hd), 97)
    k[0, T - 1] *= 3.0                                           # a dominant key in the ragged segment
    ref = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), dim=-1) @ v
    Q, K = q.half().to(U.dev()), k.half().to(U.dev())
    VT = torch.full((n, hd, ldv), float("nan"), dtype=torch.float16)
    VT[:, :, :T] = v.half().transpose(1, 2)                    # padding columns hold NaN: they must never be read
    VT = VT.to(U.dev())
    O = torch.zeros((n, T, hd), dtype=torch.float16, device=U.dev())
    rc = lib.ladi_op_attention_wide(ptr(Q), ptr(K), ptr(VT), ptr(O), hd, hd, ldv, hd, T * hd, T * hd, hd * ldv, T * hd, n, hd, T, T,
                                    1.0 / math.sqrt(hd), stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert U.rel_l2(O.float().cpu(), ref) < 3e-3, U.rel_l2(O.float().cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------ UNet forward
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods)


@pytest.mark.parametrize("hw", [(17, 15), (9, 7), (60, 80), (16, 12)])
def test_unet_forward_tiny_any_latent(tiny, hw):
    """the thresholds of test_gpu_modules.py's tiny forward (PSNR >= 55 dB, rel-L2 <= 5e-3)"""
    n, L_, D = 2, 8, tiny["ucfg"]["cross_attention_dim"]
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, 31) + hw, generator=g).half().float()
    ehs = torch.randn((n, L_, D), generator=g).half().float()
    ref = R.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, 481, ehs)
    got = tiny["mod"]["unet"](x.to(U.dev()), 481, encoder_hidden_states=ehs.to(U.dev())).sample.float().cpu()
    assert got.shape == ref.shape
    assert U.psnr(got, ref) >= 55.0 and U.rel_l2(got, ref) <= 5e-3, (U.psnr(got, ref), U.rel_l2(got, ref))


def test_unet_forward_full_small_odd_latent():
    """full-size UNet at latent 17x15 (136x120 images: levels 17x15, 9x8, 5x4, 3x2 -- every level odd or ragged, attention over 300 / 72 /
    20 / 6 tokens) and at 3x3 (levels down to 1x1), n = 2, against the restatement (rel-L2 <= 2e-3)"""
    import ladi_vton_amd as L
    ucfg = C.UNET_FULL
    sd = C.synth_state_dict(C.unet_shapes(ucfg), "unet.")
    unet = L.NativeUNet(ucfg, sd)
    for hw in ((17, 15), (3, 3)):
        g = torch.Generator().manual_seed(79)
        x = torch.randn((2, 31) + hw, generator=g).half().float()
        ehs = torch.randn((2, 77, 1024), generator=g).half().float()
        got = unet(x.to(U.dev()), 501, encoder_hidden_states=ehs.to(U.dev())).sample.float().cpu()
        with torch.no_grad():
            ref = R.unet_forward(sd, ucfg, x, 501, ehs)
        assert got.shape == ref.shape and U.rel_l2(got, ref) <= 2e-3, (hw, U.rel_l2(got, ref), U.psnr(got, ref))


def test_unet_forward_full_640x480(tiny):
    """full-size UNet at latent 80x60 (640x480 images: levels 80x60, 40x30, 20x15, 10x8): n = 2 against the restatement with the n = 16
    bound of test_gpu_e2e_golden.py (rel-L2 <= 2e-3); an n = 16 forward (other tiles, split-K choices) gives rows 0 / 7 / 15 of their n = 2 runs"""
    import ladi_vton_amd as L
    ucfg = C.UNET_FULL
    sd = C.synth_state_dict(C.unet_shapes(ucfg), "unet.")
    unet = L.NativeUNet(ucfg, sd)
    g = torch.Generator().manual_seed(78)
    x = torch.randn((16, 31, 80, 60), generator=g).half().float()
    ehs = torch.randn((16, 77, 1024), generator=g).half().float()

    def run(lo, hi):
        return unet(x[lo:hi].to(U.dev()), 501, encoder_hidden_states=ehs[lo:hi].to(U.dev())).sample.float().cpu()

    got2 = run(0, 2)
    with torch.no_grad():
        ref = R.unet_forward(sd, ucfg, x[:2], 501, ehs[:2])
    res = dict(psnr_db=round(U.psnr(got2, ref), 2), rel_l2=U.rel_l2(got2, ref))
    U.record_parity("unet_forward_full_80x60_n2_vs_anysize_ref", res)
    assert got2.shape == ref.shape and res["rel_l2"] <= 2e-3, res
    got16 = run(0, 16)
    for i, (lo, hi) in ((0, (0, 2)), (7, (7, 9)), (15, (14, 16))):
        pair = got2 if lo == 0 else run(lo, hi)
        row = pair[i - lo:i - lo + 1]
        assert U.psnr(got16[i:i + 1], row) >= 60.0, (i, U.psnr(got16[i:i + 1], row))     # fp16 forwards of different tile shapes


# ------------------------------------------------------------------------------------------------------------------ try-on loop
STEPS = 4


def _inputs(tiny, H, W):
    inp = P.synthetic_inputs(2, H, W, L=8, D=tiny["ucfg"]["cross_attention_dim"])
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    return inp


def _run(tiny, inp, H, W, fused):
    import ladi_vton_amd as L
    pipe = L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=L.DDIMScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, num_inference_steps=STEPS,
               guidance_scale=7.5, output_type="np", fused=fused, use_graph=fused,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _close(a, b):
    (img_a, lat_a), (img_b, lat_b) = a, b
    assert img_a.shape == img_b.shape and lat_a.shape == lat_b.shape
    p_img, p_lat = U.psnr(img_a, img_b, peak=1.0), U.psnr(lat_a, lat_b)
    assert p_img >= 35.0 and p_lat >= 40.0, (p_img, p_lat)


@pytest.mark.parametrize("HW", [(136, 120), (120, 200)])
def test_tryon_tiny_any_size_fused_modular_oracle(tiny, HW, monkeypatch):
    """DDIM, 4 steps, EMASC on, at image sizes whose latents (17x15, 15x25) are not multiples of 8 and whose VAE attention sees a token count
    that is not a multiple of 4 (255, 375): the fused loop (hipGraph) and the modular path each match the oracle pipeline running diffusers'
    any-size forward (image >= 35 dB, latents >= 40 dB), and each other"""
    import ladi_vton_amd as L
    H, W = HW
    inp = _inputs(tiny, H, W)
    monkeypatch.setattr(M, "unet_forward", R.unet_forward)
    ref = P.tryon_pipeline(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], inp,
                           num_inference_steps=STEPS, guidance_scale=7.5, scheduler="ddim")
    modular = _run(tiny, inp, H, W, fused=False)

    def boom(*a, **k):
        raise AssertionError("the module-by-module path ran")
    monkeypatch.setattr(L.StableDiffusionTryOnePipeline, "_run_modular", boom)
    fused = _run(tiny, inp, H, W, fused=True)
    assert fused[1].shape == (2, 4, H // 8, W // 8)
    _close(fused, ref)
    _close(modular, ref)
    _close(fused, modular)
