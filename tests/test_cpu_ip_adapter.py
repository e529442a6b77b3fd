"""The IP-Adapter image prompt without a GPU: the checkpoint key mapping (numbered and module-named), the refusals, the [2B] list handling, the
scale dict, the operator bound of tests/ip_adapter_cases.py against a float32 evaluation and against the image term's own magnitude, the
reference's self-checks (off: the plain reference's bits; on: visible at the parity thresholds the GPU tests use) and the C surface."""
import ctypes

import pytest
import torch

from ladi_vton_amd import ip_adapter as IPA
from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P
from tests import ip_adapter_cases as IC
from tests import ip_adapter_ref as R
from tests import pag_ref as PG
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import util as U

CFG = C.UNET_TINY


@pytest.fixture(scope="module")
def tiny():
    torch.set_num_threads(U.cpu_quota_threads())
    sd = C.synth_state_dict(C.unet_shapes(CFG), "unet.")
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 31, 16, 8), generator=g).half().float()
    ehs = torch.randn((2, 8, CFG["cross_attention_dim"]), generator=g).half().float()
    emb = torch.randn((2, 64), generator=g).half().float()
    return dict(sd=sd, x=x, ehs=ehs, emb=emb, ip=R.make_adapter(CFG, 4, 64))


# ------------------------------------------------------------------------------------------------------------------ the loader
def test_numbered_order_is_pinned():
    """THE table: diffusers' attn_processors order (down, up, mid), the mid block last -- index 31 of 16 blocks"""
    order = IPA.numbered_order(2)
    assert len(order) == 16 and order[-1] == "mid_block.attentions.0" and 2 * 15 + 1 == 31
    assert order[:6] == ["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(2)]
    assert order[6:15] == ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(3)]
    assert IPA.block_prefixes(2) == RU.block_prefixes(2) and sorted(order) == sorted(IPA.block_prefixes(2))


@pytest.mark.parametrize("numbered", [True, False])
@pytest.mark.parametrize("flat", [False, True])
def test_load_state_maps_every_key(tiny, numbered, flat):
    sd = R.to_diffusers(tiny["ip"], 2, numbered)
    if numbered:
        assert "31.to_k_ip.weight" in sd["ip_adapter"] and "1.to_v_ip.weight" in sd["ip_adapter"] and len(sd["ip_adapter"]) == 32
        assert torch.equal(sd["ip_adapter"]["31.to_k_ip.weight"], tiny["ip"]["mid_block.attentions.0" + R.PROC + "to_k_ip.weight"])
        assert torch.equal(sd["ip_adapter"]["13.to_v_ip.weight"], tiny["ip"]["up_blocks.1.attentions.0" + R.PROC + "to_v_ip.weight"])
    if flat:
        sd = {**{"image_proj." + k: v for k, v in sd["image_proj"].items()}, **{"ip_adapter." + k: v for k, v in sd["ip_adapter"].items()}}
    out = IPA.load_state(sd, 2)
    assert set(out) == set(tiny["ip"]) and len(out) == 36
    assert all(torch.equal(out[k], tiny["ip"][k]) for k in out)


def test_load_state_takes_library_keys_as_they_are(tiny):
    out = IPA.load_state(dict(tiny["ip"]), 2)
    assert set(out) == set(tiny["ip"])


def test_load_state_refusals(tiny):
    good = R.to_diffusers(tiny["ip"], 2, True)
    with pytest.raises(ValueError, match="several adapters"):
        IPA.load_state([good, good])
    plus = {"image_proj": {"latents": torch.zeros(1, 16, 8), "proj_in.weight": torch.zeros(8, 8), "layers.0.0.to_q.weight": torch.zeros(8, 8)},
            "ip_adapter": good["ip_adapter"]}
    with pytest.raises(ValueError, match="set_ip_tokens"):
        IPA.load_state(plus)
    faceid = {"image_proj": {"proj.0.weight": torch.zeros(8, 8), "proj.2.weight": torch.zeros(8, 8), "norm.weight": torch.zeros(8),
                             "norm.bias": torch.zeros(8)}, "ip_adapter": good["ip_adapter"]}
    with pytest.raises(ValueError, match="FaceID"):
        IPA.load_state(faceid)
    lora_proc = {"image_proj": good["image_proj"], "ip_adapter": {**good["ip_adapter"], "1.to_k_lora.down.weight": torch.zeros(4, 8)}}
    with pytest.raises(ValueError, match="FaceID"):
        IPA.load_state(lora_proc)
    missing = {"image_proj": good["image_proj"], "ip_adapter": {k: v for k, v in good["ip_adapter"].items() if not k.startswith("31.")}}
    with pytest.raises(ValueError, match="lacks 2 of 32"):
        IPA.load_state(missing)
    for bad in ("2.to_k_ip.weight", "33.to_k_ip.weight", "1.to_q_ip.weight", "foo"):
        with pytest.raises(ValueError, match="ip_adapter key"):
            IPA.load_state({"image_proj": good["image_proj"], "ip_adapter": {**good["ip_adapter"], bad: torch.zeros(1)}})
    with pytest.raises(ValueError, match="image_proj has the keys"):
        IPA.load_state({"image_proj": {"proj.weight": torch.zeros(8, 8)}, "ip_adapter": good["ip_adapter"]})
    with pytest.raises(ValueError, match="unexpected IP-Adapter key"):
        IPA.load_state({"unet.conv_in.weight": torch.zeros(1)})
    both = dict(good["ip_adapter"])
    both["mid_block.attentions.0" + R.PROC + "to_k_ip.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="same weight"):
        IPA.load_state({"image_proj": good["image_proj"], "ip_adapter": both})


# ------------------------------------------------------------------------------------------------------------------ embeddings and scales
def test_split_embeds():
    B, E = 2, 8
    pos, neg = torch.arange(B * E).float().view(B, E), -torch.arange(B * E).float().view(B, E)
    p, n = IPA.split_embeds(pos, None, B)
    assert torch.equal(p, pos) and n is None
    p, n = IPA.split_embeds(pos[:, None], neg[:, None], B)
    assert torch.equal(p, pos) and torch.equal(n, neg)
    p, n = IPA.split_embeds([torch.cat([neg, pos])[:, None]], None, B, True)           # diffusers' list: the negatives first
    assert torch.equal(p, pos) and torch.equal(n, neg)
    p, n = IPA.split_embeds([pos[:, None]], None, B, False)
    assert torch.equal(p, pos) and n is None
    with pytest.raises(ValueError, match="several adapters"):
        IPA.split_embeds([pos, pos], None, B)
    with pytest.raises(ValueError, match="already holds the negatives"):
        IPA.split_embeds([torch.cat([neg, pos])[:, None]], neg, B, True)
    with pytest.raises(ValueError, match="batch 3"):
        IPA.split_embeds(torch.zeros(3, E), None, B)
    with pytest.raises(ValueError, match=r"expected \[B, E\]"):
        IPA.split_embeds(torch.zeros(B, 4, E), None, B)
    with pytest.raises(ValueError, match="negative_ip_adapter_image_embeds"):
        IPA.split_embeds(pos, torch.zeros(B, E + 1), B)


def test_scale_list():
    assert IPA.scale_list(0.7) == [0.7] * 16 and IPA.scale_list(1) == [1.0] * 16
    got = IPA.scale_list({"down": 0.5, "mid": 1.0, "up.block_1": 0.25, "up.block_3.attentions_2": 2.0})
    want = [0.5] * 6 + [1.0] + [0.25] * 3 + [0.0] * 5 + [2.0]
    assert got == want
    assert IPA.scale_list([("down", 1.0), ("down.block_1", 0.0)]) == [1.0, 1.0, 0.0, 0.0, 1.0, 1.0] + [0.0] * 10    # later entries override
    assert IPA.scale_list({}) == [0.0] * 16
    for bad in (True, {"down.block_3": 1.0}, {"mid": float("nan")}, [("mid",)], {"side": 1.0}):
        with pytest.raises(ValueError):
            IPA.scale_list(bad)
    with pytest.raises(ValueError):
        IPA.scale_list(float("inf"))


# ------------------------------------------------------------------------------------------------------------------ the operator's bound
@pytest.mark.parametrize("c", IC.CASES, ids=IC.case_id)
def test_operator_bound(c):
    """a float32 torch evaluation stays inside the bound; the bound is at most a tenth of the image term's magnitude; the input o itself
    (a kernel that adds nothing) is outside it"""
    n, T, heads, N, pad, scale, kind = c
    case = IC.make_case(*c)
    got = IC.torch_f32(case, scale, heads)
    r = U.check_elem(got, case["ref"], case["bound"], IC.case_id(c))
    lim = (U.ulp16(case["ref"]) + case["bound"]).max().item()
    rms = case["term"].pow(2).mean().sqrt().item()
    print("%s: float32 evaluation at %.3f of the limit; largest limit %.3g, image term rms %.3g, largest |logit| %.1f"
          % (IC.case_id(c), r, lim, rms, case["max_logit"]))
    assert lim <= 0.1 * rms, (lim, rms)
    with pytest.raises(AssertionError):
        U.check_elem(case["o"], case["ref"], case["bound"], "adds nothing")
    if kind == "hot":
        assert case["max_logit"] > 40.0          # exp(40) overflows nothing in fp32, exp(2 * 40 + ..) of an unshifted sum of 16 would lose the small terms
    assert {x[1] for x in IC.CASES} >= {1, 5, 48, 768} and {x[2] for x in IC.CASES} == {5, 20} and {x[0] for x in IC.CASES} == {1, 3}
    assert {x[3] for x in IC.CASES} >= {1, 4, 5, 16, 64}


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_off_is_the_oracle_forward(tiny):
    """no image prompt, and one whose scales are all 0: oracle.models.unet_forward's bits; under PAG the zero scales change nothing either"""
    x, ehs = torch.cat([tiny["x"], tiny["x"]]), torch.cat([tiny["ehs"], tiny["ehs"]])
    tok = R.image_proj(tiny["ip"], torch.cat([tiny["emb"], tiny["emb"]]))
    assert tok.shape == (4, 4, CFG["cross_attention_dim"])
    plain = M.unet_forward(tiny["sd"], CFG, x, 481, ehs)
    assert torch.equal(RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, ip=None), plain)
    assert torch.equal(RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, ip=(tiny["ip"], tok, [0.0] * 16)), plain)
    pag = RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, pag=(PG.layer_prefixes("mid"), 2))
    assert not torch.equal(pag, plain)
    assert torch.equal(RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, pag=(PG.layer_prefixes("mid"), 2), ip=(tiny["ip"], tok, [0.0] * 16)), pag)


def test_reference_image_term_is_visible(tiny):
    """scale 1 in every block: below the 55 dB the GPU forward test asks against the reference; the mid block alone too is another function"""
    x, ehs = tiny["x"], tiny["ehs"]
    tok = R.image_proj(tiny["ip"], tiny["emb"])
    plain = M.unet_forward(tiny["sd"], CFG, x, 481, ehs)
    on = RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, ip=(tiny["ip"], tok, [1.0] * 16))
    mid = RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, ip=(tiny["ip"], tok, [0.0] * 6 + [1.0] + [0.0] * 9))
    p, pm = U.psnr(on, plain), U.psnr(mid, plain)
    print("reference forward with the image term against plain: %.1f dB (mid block alone %.1f dB)" % (p, pm))
    assert torch.isfinite(on).all() and p < 55.0, p
    assert pm < 55.0 and not torch.equal(mid, on), pm
    # the tokens matter, not only the adapter: other embeddings give another output
    other = RU.unet_forward(tiny["sd"], CFG, x, 481, ehs, ip=(tiny["ip"], R.image_proj(tiny["ip"], -tiny["emb"]), [1.0] * 16))
    assert U.psnr(other, on) < 55.0


def test_reference_loop_is_not_the_plain_loop(tiny):
    """4 DDIM steps at 64x48: the latents are below the 40 dB the GPU loop test asks against the reference; with all scales 0 the loop is
    the one without an image prompt, and with the oracle's own scheduler, at a size the oracle runs, that is oracle.pipeline.tryon_pipeline"""
    vcfg = C.VAE_TINY
    vsd = C.synth_state_dict(C.vae_shapes(vcfg), "vae.")
    inp = P.synthetic_inputs(2, 64, 48, L=8, D=CFG["cross_attention_dim"])
    _, plain = RT.tryon_reference(tiny["sd"], CFG, vsd, vcfg, None, inp, 4, "ddim")
    counts = {}
    _, on = RT.tryon_reference(tiny["sd"], CFG, vsd, vcfg, None, inp, 4, "ddim", ip=(tiny["ip"], tiny["emb"], None, [1.0] * 16), info=counts)
    _, zero = RT.tryon_reference(tiny["sd"], CFG, vsd, vcfg, None, inp, 4, "ddim", ip=(tiny["ip"], tiny["emb"], None, [0.0] * 16))
    inp8 = P.synthetic_inputs(2, 64, 64, L=8, D=CFG["cross_attention_dim"])          # latents 8x8: a size the oracle runs
    img_o, lat_o = P.tryon_pipeline(tiny["sd"], CFG, vsd, vcfg, None, inp8, num_inference_steps=4, guidance_scale=7.5, scheduler="ddim")
    img_z, lat_z = RT.tryon_reference(tiny["sd"], CFG, vsd, vcfg, None, inp8, 4, P.make_scheduler("ddim"), ip=(tiny["ip"], tiny["emb"], None, [0.0] * 16))
    assert torch.equal(lat_z, lat_o) and torch.equal(img_z, img_o)
    p = U.psnr(on, plain)
    print("reference loop with the image term against plain: latents %.1f dB" % p)
    assert counts["evals"] == 4 and torch.isfinite(on).all() and p < 40.0, p
    assert torch.equal(zero, plain)


# ------------------------------------------------------------------------------------------------------------------ the C surface
NEW_SYMBOLS = ["ladi_unet_ip_adapter_load", "ladi_unet_ip_adapter_unload", "ladi_unet_ip_adapter_info", "ladi_unet_set_ip_scale",
               "ladi_unet_ip_scale", "ladi_unet_set_ip_context", "ladi_unet_set_ip_tokens", "ladi_unet_clear_ip_context",
               "ladi_unet_set_ip_route", "ladi_tryon_set_ip_adapter", "ladi_op_ip_attn_add"]


def test_symbols_are_declared_and_refuse_null_handles():
    from ladi_vton_amd import _lib
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert getattr(lib, s).argtypes is not None and len(getattr(lib, s).argtypes) == len(_lib.SIGNATURES[s][1]), s
    one = (ctypes.c_float * 16)(*[1.0] * 16)
    assert lib.ladi_unet_set_ip_scale(None, one, 16) == -1 and "ladi_unet_set_ip_scale" in _lib.last_error()
    assert lib.ladi_unet_ip_adapter_load(None, None) != 0 and "ladi_unet_ip_adapter_load" in _lib.last_error()
    assert lib.ladi_unet_ip_adapter_unload(None) != 0 and lib.ladi_unet_clear_ip_context(None) == -1
    assert lib.ladi_unet_set_ip_context(None, None, 1, None) != 0 and lib.ladi_unet_set_ip_tokens(None, None, 1, 4, None) != 0
    assert lib.ladi_tryon_set_ip_adapter(None, None, None) == -1 and "ladi_tryon_set_ip_adapter" in _lib.last_error()
    buf = (ctypes.c_uint16 * 4096)()
    v = ctypes.cast(buf, ctypes.c_void_p).value
    v += (-v) % 16
    v = ctypes.c_void_p(v)
    run = lambda N, ldo=64, q=v: lib.ladi_op_ip_attn_add(q, 64, 64, v, 128, 128, v, 128, 128, v, ldo, 64, 1, 1, 1, N, 1.0, None)
    assert run(0) == -1 and "N = 0" in _lib.last_error()            # refused before any launch: no GPU is needed to see it
    assert run(65) == -1 and "N = 65" in _lib.last_error()
    assert run(4, ldo=68) == -1 and run(4, ldo=32) == -1 and run(4, q=None) == -1


def test_pipeline_argument_checks():
    """what the pipeline refuses before any native call: a UNet without the interface, negatives without embeddings"""
    import ladi_vton_amd as L
    from types import SimpleNamespace
    pipe = L.StableDiffusionTryOnePipeline.__new__(L.StableDiffusionTryOnePipeline)
    pipe.unet = SimpleNamespace()
    for call in (lambda: pipe.load_ip_adapter({}), lambda: pipe.unload_ip_adapter(), lambda: pipe.set_ip_adapter_scale(1.0)):
        with pytest.raises(ValueError, match="NativeUNet"):
            call()
