"""IP-Adapter from a picture, without a GPU: the loader's handling of Plus (Resampler) checkpoints, the refusals of the library's own check
(ladi_resampler_create refuses on the host, before it asks for a device), the C surface, and the conditions that keep
tests/test_gpu_ip_image.py honest -- all computed from the reference (tests/ip_image_ref.py) alone: a wrong tap, swapped groups or an absent
term would fail the GPU thresholds, and an fp16-storing implementation can reach them."""
import ctypes
import os
import re

import pytest
import torch

from ladi_vton_amd import configs as LC
from ladi_vton_amd import ip_adapter as IPA
from oracle import configs as C
from oracle import vision as V
from tests import ip_adapter_ref as R
from tests import ip_image_ref as IR
from tests import ref_unet as RU
from tests import util as U

CFG = C.UNET_TINY
VCFG = C.VISION_TINY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plus():
    torch.set_num_threads(U.cpu_quota_threads())
    return IR.make_plus_adapter(CFG, 320, 128, 2, 2, 16)


@pytest.fixture(scope="module")
def vision():
    torch.set_num_threads(U.cpu_quota_threads())
    sd = C.synth_state_dict({**C.vision_shapes(VCFG), **LC.vision_projection_shapes(VCFG, 64)}, "vision.")
    px = torch.randn((3, 3, 56, 56), generator=torch.Generator().manual_seed(5)).half().float()
    return dict(sd=sd, px=px)


# ------------------------------------------------------------------------------------------------------------------ the loader
@pytest.mark.parametrize("numbered", [True, False])
@pytest.mark.parametrize("flat", [False, True])
def test_load_state_maps_a_complete_resampler(plus, numbered, flat):
    sd = R.to_diffusers(plus, 2, numbered)
    assert set(sd["image_proj"]) == set(IPA.resampler_keys(2)) and len(sd["image_proj"]) == 7 + 2 * 11
    if flat:
        sd = {**{"image_proj." + k: v for k, v in sd["image_proj"].items()}, **{"ip_adapter." + k: v for k, v in sd["ip_adapter"].items()}}
    out = IPA.load_state(sd, 2)
    assert set(out) == set(plus) and len(out) == 29 + 32
    assert all(torch.equal(out[k], plus[k]) for k in out)
    assert set(IPA.load_state(dict(plus), 2)) == set(plus)          # the library's keys as they are
    info = IPA.check_resampler(IR.resampler_of(plus), 64)
    assert info == dict(N=16, E=320, dim=128, depth=2, inner=128, out_dim=128)


def test_load_state_refuses_what_is_not_a_complete_resampler(plus):
    good = R.to_diffusers(plus, 2, True)
    rs = good["image_proj"]
    load = lambda proj: IPA.load_state({"image_proj": proj, "ip_adapter": good["ip_adapter"]})
    for gone in ("latents", "norm_out.bias", "layers.1.1.3.weight", "layers.0.0.to_kv.weight"):
        with pytest.raises(ValueError, match="set_ip_tokens") as e:
            load({k: v for k, v in rs.items() if k != gone})
        assert "lacks 1 of 29" in str(e.value) and gone in str(e.value)
    with pytest.raises(ValueError, match="lacks 11 of 18 keys, e.g. 'layers.0.0.norm1.bias'"):      # a hole in the numbering: layer 1 without layer 0
        load({k: v for k, v in rs.items() if not k.startswith("layers.0.")})
    with pytest.raises(ValueError, match="unexpected key 'layers.0.0.to_q.bias'"):
        load({**rs, "layers.0.0.to_q.bias": torch.zeros(128)})
    with pytest.raises(ValueError, match="unexpected key 'perceiver_resampler"):
        load({**rs, "perceiver_resampler.proj_in.weight": torch.zeros(8, 8)})
    with pytest.raises(ValueError, match=r"layers.1.0.to_kv.weight has shape \[128, 128\], expected \[256, 128\]"):
        load({**rs, "layers.1.0.to_kv.weight": torch.zeros(128, 128)})
    with pytest.raises(ValueError, match=r"latents has shape \(16, 128\)"):
        load({**rs, "latents": torch.zeros(16, 128)})
    with pytest.raises(ValueError, match="65 latents"):
        load({**rs, "latents": torch.zeros(1, 65, 128)})
    with pytest.raises(ValueError, match="no multiple of dim_head 96"):
        IPA.check_resampler(rs, 96)
    with pytest.raises(ValueError, match="dim_head 32"):
        IPA.check_resampler(rs, 32)
    # FaceID and several adapters: as before
    with pytest.raises(ValueError, match="several adapters"):
        IPA.load_state([good, good])
    with pytest.raises(ValueError, match="FaceID"):
        IPA.load_state({"image_proj": rs, "ip_adapter": {**good["ip_adapter"], "1.to_k_lora.down.weight": torch.zeros(4, 8)}})


def _create(sd, dim_head=64):
    """ladi_resampler_create on the host -> (handle or None, message)"""
    from ladi_vton_amd import _lib
    from ladi_vton_amd.modules import _Weights
    lib = _lib.load()
    with _Weights(sd) as w:
        h = lib.ladi_resampler_create(w.h, dim_head)
    msg = _lib.last_error()
    if h:
        lib.ladi_resampler_destroy(h)
    return h, msg


def test_library_refuses_on_the_host(plus):
    """every limit of the header, checked by ladi_resampler_create before it asks for a device: each refusal names its cause"""
    rs = IR.resampler_of(plus)
    z = torch.zeros
    cases = [({**rs, "latents": z(1, 65, 128)}, 64, "65 latents"),
             ({k: v for k, v in rs.items() if k != "latents"}, 64, "'latents' is missing"),
             (rs, 96, "no multiple of dim_head 96"),
             (rs, 32, "dim_head 32 is not one of 64, 80, 96, 128"),
             ({**rs, "proj_in.weight": z(128, 324)}, 64, "multiples of 8"),
             ({**rs, "layers.0.0.to_out.weight": z(128, 64)}, 64, "layers.0.0.to_out.weight of shape [128, 64] is not [128, 128]"),
             ({**rs, "layers.1.1.0.bias": z(64)}, 64, "layers.1.1.0.bias does not have 128 entries"),
             ({**rs, "layers.0.0.to_q.bias": z(128)}, 64, "unexpected key 'layers.0.0.to_q.bias'"),
             ({k: v for k, v in rs.items() if not k.startswith("layers.")}, 64, "layers.0.0.to_q.weight' is missing"),
             ({k: v for k, v in rs.items() if k != "layers.1.1.3.weight"}, 64, "'layers.1.1.3.weight' is missing")]
    for sd, dh, text in cases:
        h, msg = _create(sd, dh)
        assert not h and "ladi_resampler_create" in msg and text in msg, (text, msg)


# ------------------------------------------------------------------------------------------------------------------ the C surface
NEW_SYMBOLS = ["ladi_vision_encoder_projection_dim", "ladi_vision_encoder_forward_ex", "ladi_resampler_create", "ladi_resampler_destroy",
               "ladi_resampler_info", "ladi_resampler_forward", "ladi_unet_ip_adapter_load_ex", "ladi_unet_ip_adapter_is_plus",
               "ladi_unet_set_ip_context_seq", "ladi_tryon_set_ip_adapter_seq"]


def test_symbols_are_declared_and_refuse_null_handles():
    from ladi_vton_amd import _lib
    header = open(os.path.join(ROOT, "include", "ladi_native.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
        m = re.search(r"\b%s\(([^;]*)\);" % s, header)
        assert m, "%s is not declared in include/ladi_native.h" % s
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[s][1]), s          # the header and ctypes agree on the argument count
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert len(getattr(lib, s).argtypes) == len(_lib.SIGNATURES[s][1]), s
    assert lib.ladi_vision_encoder_projection_dim(None) == -1 and "ladi_vision_encoder_projection_dim" in _lib.last_error()
    assert lib.ladi_vision_encoder_forward_ex(None, None, 1, 1, None, None, None, None, None) != 0
    assert "ladi_vision_encoder_forward_ex" in _lib.last_error()
    assert not lib.ladi_resampler_create(None, 64) and "ladi_resampler_create" in _lib.last_error()
    lib.ladi_resampler_destroy(None)
    assert lib.ladi_resampler_info(None, None, None, None, None, None, None) == -1 and "ladi_resampler_info" in _lib.last_error()
    assert lib.ladi_resampler_forward(None, None, 1, 1, None, None) != 0 and "ladi_resampler_forward" in _lib.last_error()
    assert lib.ladi_unet_ip_adapter_load_ex(None, None, 64) != 0 and "ladi_unet_ip_adapter_load_ex" in _lib.last_error()
    assert lib.ladi_unet_ip_adapter_is_plus(None) == -1
    assert lib.ladi_unet_set_ip_context_seq(None, None, 1, 1, None) != 0 and "ladi_unet_set_ip_context_seq" in _lib.last_error()
    assert lib.ladi_tryon_set_ip_adapter_seq(None, None, None, 1) == -1 and "ladi_tryon_set_ip_adapter_seq" in _lib.last_error()
    assert "#define LADI_TRYON_IP_ADAPTER_KIND (-19)" in header


def test_pipeline_refusals_need_no_gpu():
    """what the pipeline refuses before any native call: pictures that are no [B, 3, H, W] tensor or PIL images, encode_image without an encoder;
    Plus hidden states through split_embeds"""
    import ladi_vton_amd as L
    pipe = L.StableDiffusionTryOnePipeline.__new__(L.StableDiffusionTryOnePipeline)
    assert pipe.image_encoder is None
    with pytest.raises(ValueError, match="image_encoder"):
        pipe.encode_image(torch.zeros(1, 3, 8, 8))
    for bad in (torch.zeros(3, 8, 8), torch.zeros(1, 4, 8, 8), "garment.png", []):
        with pytest.raises(ValueError, match="ip_adapter_image"):
            pipe._ip_image_tensor(bad)
    from PIL import Image
    t = pipe._ip_image_tensor([Image.new("RGB", (6, 8), (255, 0, 127)), Image.new("L", (6, 8), 255)])
    assert t.shape == (2, 3, 8, 6) and t.dtype == torch.float32 and float(t.max()) == 1.0 and float(t.min()) == -1.0
    with pytest.raises(ValueError, match="different sizes"):
        pipe._ip_image_tensor([Image.new("RGB", (6, 8)), Image.new("RGB", (8, 8))])
    pipe.image_encoder = object()
    pipe._ip_uncond = "stale"
    pipe.image_encoder = object()
    assert pipe._ip_uncond is None                                   # a new encoder drops the cached unconditional states
    B, T, E = 2, 5, 8
    pos, neg = torch.arange(B * T * E).float().view(B, T, E), -torch.arange(B * T * E).float().view(B, T, E)
    p, n = IPA.split_embeds(pos, neg, B, seq=True)
    assert torch.equal(p, pos) and torch.equal(n, neg)
    p, n = IPA.split_embeds([torch.cat([neg, pos])], None, B, True, seq=True)     # diffusers' list: the negatives first
    assert torch.equal(p, pos) and torch.equal(n, neg)
    with pytest.raises(ValueError, match="Plus adapter"):
        IPA.split_embeds(pos[:, 0], None, B, seq=True)
    with pytest.raises(ValueError, match="batch 3"):
        IPA.split_embeds(torch.zeros(3, T, E), None, B, seq=True)
    with pytest.raises(ValueError, match=r"expected \[B, E\]"):
        IPA.split_embeds(pos, None, B)                                 # a plain adapter still refuses sequences


def test_vision_projection_shapes_leave_vision_shapes_alone():
    base = C.vision_shapes(C.VISION_FULL)
    assert "visual_projection.weight" not in base
    assert LC.vision_projection_shapes(C.VISION_FULL, 1024) == {"visual_projection.weight": (1024, 1280)}


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def test_reference_pieces(vision, plus):
    """the identity-projection device gives the Plus tokens exactly; the penultimate state is the last layer's input: running the last
    layer on it gives last_hidden_state"""
    hidden = IR.penultimate(vision["sd"], VCFG, vision["px"])
    last, pooled = V.clip_vision_forward(vision["sd"], VCFG, vision["px"])
    assert hidden.shape == last.shape == (3, 17, 320) and not torch.equal(hidden, last)
    # one layer: the pre_layrnorm output, which is also what the two-layer encoder's first layer reads
    pre_ln = IR.penultimate(vision["sd"], dict(VCFG, layers=1), vision["px"])
    assert torch.equal(V.clip_vision_forward(vision["sd"], dict(VCFG, layers=1), vision["px"])[0], hidden) and not torch.equal(pre_ln, hidden)
    assert IR.image_embeds(vision["sd"], VCFG, vision["px"]).shape == (3, 64)
    tok = IR.resampler_forward(IR.resampler_of(plus), hidden, 2)
    assert tok.shape == (3, 16, 128) and torch.isfinite(tok).all()
    via_plain = R.image_proj(IR.as_plain(plus), IR.plain_embeds(plus, hidden, 2))
    assert torch.equal(via_plain, tok)


# ------------------------------------------------------------------------------------------------------------------ honesty conditions
def test_a_wrong_tap_would_fail(vision, plus):
    """(a) tokens from hidden_states[-1] against tokens from [-2]: below the module test's 50 dB"""
    rs = IR.resampler_of(plus)
    pen = IR.penultimate(vision["sd"], VCFG, vision["px"])
    last, _ = V.clip_vision_forward(vision["sd"], VCFG, vision["px"])
    p_states, p_tok = U.psnr(last, pen), U.psnr(IR.resampler_forward(rs, last, 2), IR.resampler_forward(rs, pen, 2))
    print("hidden_states[-1] against [-2]: states %.1f dB, tokens %.1f dB" % (p_states, p_tok))
    assert p_states < IR.MODULE_PSNR and p_tok < IR.MODULE_PSNR


def test_swapped_groups_would_fail(vision, plus):
    """(b) the tokens of the picture against the tokens of the zero picture (the unconditional group): below 50 dB"""
    rs = IR.resampler_of(plus)
    cond = IR.resampler_forward(rs, IR.penultimate(vision["sd"], VCFG, vision["px"]), 2)
    unc = IR.resampler_forward(rs, IR.penultimate(vision["sd"], VCFG, torch.zeros_like(vision["px"])), 2)
    p = U.psnr(unc, cond)
    print("uncond tokens against cond tokens: %.1f dB" % p)
    assert p < IR.MODULE_PSNR


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_an_absent_term_would_fail(plus, hw):
    """(c) the reference UNet forward with Plus tokens against the plain forward: below the 55 dB of the forward test"""
    sd = C.synth_state_dict(C.unet_shapes(CFG), "unet.")
    x, ehs, hidden = IR.unet_case(CFG, 4, *hw)
    tok = IR.resampler_forward(IR.resampler_of(plus), hidden, 2)
    on = RU.unet_forward(sd, CFG, x, 481, ehs, ip=(plus, tok, [1.0] * 16))
    p = U.psnr(on, RU.unet_forward(sd, CFG, x, 481, ehs))        # (the any-size reference: the oracle's own forward needs sides of 8)
    print("reference forward with Plus tokens against plain at %dx%d: %.1f dB" % (hw + (p,)))
    assert torch.isfinite(on).all() and p < 55.0


def test_an_absent_term_would_fail_the_loop(vision, plus):
    """(c) the reference loop (B = 2, 64x48, 4 DDIM steps) with the picture's image prompt against the plain loop: latents below the 40 dB of
    the loop test, for the Plus and for the plain adapter; another picture gives other latents (a stale context would show)"""
    from oracle import pipeline as P
    from tests import ref_tryon as RT
    vcfg = C.VAE_TINY
    sd, vsd = C.synth_state_dict(C.unet_shapes(CFG), "unet."), C.synth_state_dict(C.vae_shapes(vcfg), "vae.")
    inp = P.synthetic_inputs(2, 64, 48, L=8, D=CFG["cross_attention_dim"])
    loop = lambda ip: RT.tryon_reference(sd, CFG, vsd, vcfg, None, inp, 4, "ddim", ip=ip)[1]
    base = loop(None)
    pic = IR.pictures(2)
    lat_plus = loop(IR.loop_ip(plus, vision["sd"], VCFG, pic, heads=2))
    lat_plain = loop(IR.loop_ip(R.make_adapter(CFG, 4, 64), vision["sd"], VCFG, pic))
    lat_other = loop(IR.loop_ip(plus, vision["sd"], VCFG, IR.pictures(2, seed=1), heads=2))
    p1, p2, p3 = U.psnr(lat_plus, base), U.psnr(lat_plain, base), U.psnr(lat_other, lat_plus)
    print("reference loop against plain: Plus %.1f dB, plain adapter %.1f dB; another picture against the first %.1f dB" % (p1, p2, p3))
    assert torch.isfinite(lat_plus).all() and p1 < 40.0 and p2 < 40.0 and p3 < 40.0


@pytest.mark.parametrize("c", IR.RESAMPLER_CASES, ids=IR.case_id)
def test_thresholds_are_reachable(c):
    """(d) the reference with every Linear / LayerNorm / attention output rounded to fp16 stays inside the module contract"""
    sd = IR.make_resampler(*c[2:])
    x = IR.case_input(c)
    ref, r16 = IR.resampler_forward(sd, x, c[4]), IR.resampler_forward(sd, x, c[4], round16=True)
    p, e = U.psnr(r16, ref), U.rel_l2(r16, ref)
    print("%s: fp16-rounded reference %.1f dB, rel-L2 %.2e" % (IR.case_id(c), p, e))
    assert ref.shape == (c[0], c[6], c[7]) and p >= IR.MODULE_PSNR + 6.0 and e <= IR.MODULE_REL_L2 / 2


def test_forward_and_loop_thresholds_are_reachable(vision, plus):
    """(d) for the UNet forward (55 dB, rel-L2 5e-3) and the loop (latents 40 dB, image 35 dB): the references fed Plus tokens from the
    fp16-rounded Resampler (and, for the loop, fp16-rounded encoder states) against the same references fed the fp32 ones"""
    from oracle import pipeline as P
    from tests import ref_tryon as RT
    sd = C.synth_state_dict(C.unet_shapes(CFG), "unet.")
    rs = IR.resampler_of(plus)
    for hw in ((32, 24), (26, 19)):
        x, ehs, hidden = IR.unet_case(CFG, 4, *hw)
        run = lambda tok: RU.unet_forward(sd, CFG, x, 481, ehs, ip=(plus, tok, [1.0] * 16))
        ref, r16 = run(IR.resampler_forward(rs, hidden, 2)), run(IR.resampler_forward(rs, hidden, 2, round16=True))
        p, e = U.psnr(r16, ref), U.rel_l2(r16, ref)
        print("forward %dx%d with fp16-rounded tokens: %.1f dB, rel-L2 %.2e" % (hw + (p, e)))
        assert p >= 55.0 + 6.0 and e <= 5e-3 / 2
    vcfg = C.VAE_TINY
    vsd = C.synth_state_dict(C.vae_shapes(vcfg), "vae.")
    inp = P.synthetic_inputs(2, 64, 48, L=8, D=CFG["cross_attention_dim"])
    adapter, cond, unc, scales = IR.loop_ip(plus, vision["sd"], VCFG, IR.pictures(2), heads=2)
    px = IR.clip_pixels(IR.pictures(2), VCFG["image_size"])
    pre16 = lambda states: IR.resampler_forward(rs, states.half().float(), 2, round16=True, return_prenorm=True)[1].reshape(states.shape[0], -1)
    cond16 = pre16(IR.penultimate(vision["sd"], VCFG, px))
    unc16 = pre16(IR.penultimate(vision["sd"], VCFG, torch.zeros_like(px[:1]))).expand(2, -1).contiguous()
    loop = lambda c, u: RT.tryon_reference(sd, CFG, vsd, vcfg, None, inp, 4, "ddim", ip=(adapter, c, u, scales))
    (img, lat), (img16, lat16) = loop(cond, unc), loop(cond16, unc16)
    p_lat, p_img = U.psnr(lat16, lat), U.psnr(img16, img, peak=1.0)
    print("loop with fp16-rounded states and tokens: latents %.1f dB, image %.1f dB" % (p_lat, p_img))
    assert p_lat >= 40.0 + 6.0 and p_img >= 35.0 + 6.0


def test_vision_thresholds_are_reachable(vision):
    """(d) for the encoder's new outputs: the image embeddings from fp16-rounded pooled output and weights stay inside the contract"""
    ref = IR.image_embeds(vision["sd"], VCFG, vision["px"])
    pooled = V.clip_vision_forward(vision["sd"], VCFG, vision["px"])[1].half().float()
    r16 = torch.nn.functional.linear(pooled, vision["sd"]["visual_projection.weight"]).half().float()
    assert U.psnr(r16, ref) >= IR.MODULE_PSNR + 6.0 and U.rel_l2(r16, ref) <= IR.MODULE_REL_L2 / 2
