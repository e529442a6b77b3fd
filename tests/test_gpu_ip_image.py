"""IP-Adapter from a picture on the device: the vision encoder's hidden_states[-2] and image_embeds (ladi_vision_encoder_forward_ex), the
Resampler module, the native UNet's forward through a loaded Plus adapter, and the tiny model end to end with `ip_adapter_image=` (fused
hipGraph, fused eager, modular, lanes, PAG, a second picture on captured graphs, the misuse) -- each against tests/ip_image_ref.py at the
project's module, forward and loop contracts, in poisoned buffers where the entry takes raw pointers.  tests/test_cpu_ip_image.py shows from the reference alone
that a wrong tap, swapped groups or an absent term would fail these thresholds and that an fp16-storing implementation can reach them."""
import ctypes

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd import configs as LC
from ladi_vton_amd._lib import stream_ptr
from oracle import configs as C
from oracle import vision as V
from tests import ip_adapter_ref as R
from tests import ip_image_ref as IR
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import tiny_tryon as TT
from tests import util as U

pytestmark = pytest.mark.gpu
VCFG = C.VISION_TINY
P = ctypes.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _module_close(what, got, ref, key=None):
    ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
    print("%s: PSNR %.2f dB, rel-L2 %.3g" % (what, ps, rl))
    if key:
        U.record_parity(key, dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert ps >= IR.MODULE_PSNR and rl <= IR.MODULE_REL_L2, (what, ps, rl)


# ------------------------------------------------------------------------------------------------------------------ the vision encoder
@pytest.fixture(scope="module")
def vision():
    sd = C.synth_state_dict({**C.vision_shapes(VCFG), **LC.vision_projection_shapes(VCFG, 64)}, "vision.")
    px = torch.randn((3, 3, 56, 56), generator=torch.Generator().manual_seed(5)).half().float()
    return dict(sd=sd, px=px, pxd=px.to(U.dev()))


def _outs(B, T=17, H=320, Pd=64):
    return dict(hidden=U.guarded_out(B * T, H), pooled=U.guarded_out(B, H), pen=U.guarded_out(B * T, H), emb=U.guarded_out(B, Pd))


def _forward_ex(lib, enc, pxd, o, which=("hidden", "pooled", "pen", "emb")):
    a = [P(o[k].ptr) if k in which else None for k in ("hidden", "pooled", "pen", "emb")]
    rc = lib.ladi_vision_encoder_forward_ex(enc.h, P(pxd.data_ptr()), _lib.dtype_code(pxd), pxd.shape[0], a[0], a[1], a[2], a[3], stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("layers", [2, 1])
def test_vision_forward_ex(lib, vision, layers):
    """B = 3 on VISION_TINY (17 tokens, 4 heads of 80) with 2 layers and with 1: penultimate states and image embeddings against the
    reference at the module contract; hidden and pooled are ladi_vision_encoder_forward's bits; every subset of outputs gives the same
    bits and touches nothing else"""
    import ladi_vton_amd as L
    cfg = dict(VCFG, layers=layers)
    enc = L.NativeCLIPVisionEncoder(cfg, vision["sd"])
    assert enc.projection_dim == 64
    o = _outs(3)
    assert _forward_ex(lib, enc, vision["pxd"], o) == 0, _lib.last_error()
    for k, g in o.items():
        U.assert_untouched(g, "forward_ex " + k)
    tag = "vision_ex_tiny_l%d" % layers
    _module_close("penultimate, %d layers" % layers, o["pen"].cpu().float().reshape(3, 17, 320), IR.penultimate(vision["sd"], cfg, vision["px"]), tag + "_pen")
    _module_close("image_embeds, %d layers" % layers, o["emb"].cpu().float(), IR.image_embeds(vision["sd"], cfg, vision["px"]), tag + "_emb")
    ref_h, ref_p = V.clip_vision_forward(vision["sd"], cfg, vision["px"])
    _module_close("last_hidden_state, %d layers" % layers, o["hidden"].cpu().float().reshape(3, 17, 320), ref_h)
    hid, pool = torch.empty((3, 17, 320), dtype=torch.float16, device=U.dev()), torch.empty((3, 320), dtype=torch.float16, device=U.dev())
    assert lib.ladi_vision_encoder_forward(enc.h, P(vision["pxd"].data_ptr()), _lib.F32, 3, P(hid.data_ptr()), P(pool.data_ptr()), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(hid.cpu().reshape(51, 320)), _bits(o["hidden"].cpu())) and torch.equal(_bits(pool.cpu()), _bits(o["pooled"].cpu()))
    # subsets: each output alone, and pairs that share a stage; NULL outputs are not written, the others keep their bits
    for which in (("hidden",), ("pooled",), ("pen",), ("emb",), ("pen", "emb"), ("hidden", "pen")):
        s = _outs(3)
        before = {k: _bits(g.buf.cpu()) for k, g in s.items()}
        assert _forward_ex(lib, enc, vision["pxd"], s, which) == 0, (which, _lib.last_error())
        for k, g in s.items():
            if k in which:
                U.assert_untouched(g, "forward_ex %s of %s" % (k, which))
                assert torch.equal(_bits(g.cpu()), _bits(o[k].cpu())), (which, k)
            else:
                assert torch.equal(_bits(g.buf.cpu()), before[k]), (which, k)
    assert _forward_ex(lib, enc, vision["pxd"], _outs(3), ()) == 0                  # all NULL: accepted, nothing to do
    # the Python surface
    out = enc(vision["pxd"], output_hidden_states=True)
    torch.cuda.synchronize()
    assert len(out.hidden_states) == layers + 1 and all(h is None for h in out.hidden_states[:-2])
    assert torch.equal(_bits(out.hidden_states[-2].cpu().reshape(51, 320)), _bits(o["pen"].cpu()))
    assert out.hidden_states[-1] is out.last_hidden_state and torch.equal(_bits(out.last_hidden_state.cpu().reshape(51, 320)), _bits(o["hidden"].cpu()))
    assert torch.equal(_bits(out.image_embeds.cpu()), _bits(o["emb"].cpu())) and torch.equal(_bits(out.pooler_output.cpu()), _bits(o["pooled"].cpu()))
    assert enc(vision["pxd"]).hidden_states is None and enc(vision["pxd"]).image_embeds is not None


def test_vision_image_embeds_need_a_projection(lib, vision):
    """without visual_projection.weight: projection_dim 0, image_embeds None, and asking forward_ex for them is an error that writes nothing"""
    import ladi_vton_amd as L
    enc = L.NativeCLIPVisionEncoder(VCFG, {k: v for k, v in vision["sd"].items() if not k.startswith("visual_projection")})
    assert enc.projection_dim == 0
    o = _outs(3)
    before = {k: _bits(g.buf.cpu()) for k, g in o.items()}
    rc = _forward_ex(lib, enc, vision["pxd"], o)
    assert rc != 0 and "visual_projection" in _lib.last_error()
    for k, g in o.items():
        assert torch.equal(_bits(g.buf.cpu()), before[k]), k
    out = enc(vision["pxd"], output_hidden_states=True)
    assert out.image_embeds is None and out.hidden_states[-2] is not None
    full = L.NativeCLIPVisionEncoder(VCFG, vision["sd"])                          # the projection changes nothing else
    assert torch.equal(_bits(full(vision["pxd"]).last_hidden_state.cpu()), _bits(enc(vision["pxd"]).last_hidden_state.cpu()))


# ------------------------------------------------------------------------------------------------------------------ the Resampler
@pytest.mark.parametrize("c", IR.RESAMPLER_CASES, ids=IR.case_id)
def test_resampler_module(lib, c):
    """NativeResampler against the fp32 reference at the module contract; the input is read only, nothing outside the output view is written,
    two launches are bit-equal"""
    import ladi_vton_amd as L
    n, T, E, dim, heads, depth, N, out_dim = c
    sd = IR.make_resampler(*c[2:])
    rs = L.NativeResampler(sd, dim_head=dim // heads)
    assert (rs.num_queries, rs.embedding_dim, rs.dim, rs.depth, rs.heads, rs.output_dim) == (N, E, dim, depth, heads, out_dim)
    x = IR.case_input(c)
    outs = []
    for _ in range(2):
        gx, go = U.guarded(x.half().reshape(n * T, E)), U.guarded_out(n * N, out_dim)
        rc = lib.ladi_resampler_forward(rs.h, P(gx.ptr), n, T, P(go.ptr), stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        U.assert_untouched(gx, "resampler input")
        U.assert_untouched(go, "resampler output")
        assert torch.equal(_bits(gx.cpu()), _bits(x.half().reshape(n * T, E)))
        outs.append(go.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    _module_close("resampler " + IR.case_id(c), outs[0].float().reshape(n, N, out_dim), IR.resampler_forward(sd, x, heads), "resampler_" + IR.case_id(c))
    assert torch.equal(_bits(rs(x.to(U.dev())).cpu().reshape(n * N, out_dim)), _bits(outs[0]))
    with pytest.raises(ValueError, match="expected"):
        rs(torch.zeros((n, T, E + 8)))
    assert lib.ladi_resampler_forward(rs.h, P(gx.ptr), 0, T, P(go.ptr), stream_ptr()) != 0 and ">= 1" in _lib.last_error()
    assert lib.ladi_resampler_forward(rs.h, None, n, T, P(go.ptr), stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481
ONES = [1.0] * 16
GEO = dict(E=320, dim=128, heads=2, depth=2, N=16)


@pytest.fixture(scope="module")
def tiny():
    t = TT.build()
    plus = IR.make_plus_adapter(t["ucfg"], **GEO)
    t["mod"]["unet"].load_ip_adapter(R.to_diffusers(plus, 2, numbered=True), image_proj_dim_head=64)      # diffusers' nested layout, numbered keys
    t.update(plus=plus)
    yield t


@pytest.mark.parametrize("hw", [(32, 24), (26, 19)])
def test_unet_forward_through_a_plus_adapter(tiny, hw):
    """NativeUNet tiny, n = 4, t = 481: hidden states [4, 17, 320] through the loaded Resampler against ref_unet.unet_forward with the
    reference's tokens (PSNR >= 55 dB, rel-L2 <= 5e-3, as test_forward_vs_reference); the bits of ip_tokens= with NativeResampler's tokens;
    another function than the plain forward; every scale 0 and no context are the plain forward bit for bit"""
    import ladi_vton_amd as L
    unet = tiny["mod"]["unet"]
    assert unet.ip_adapter_info == (16, 320) and unet.ip_adapter_is_plus and unet.ip_adapter_scale == ONES
    x, ehs, hidden = IR.unet_case(tiny["ucfg"], 4, *hw)
    xd, ed, hd = x.to(U.dev()), ehs.to(U.dev()), hidden.to(U.dev())
    run = lambda **kw: unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu()
    plain = run()
    on = run(ip_image_embeds=hd)
    tok = IR.resampler_forward(IR.resampler_of(tiny["plus"]), hidden, GEO["heads"])
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, ip=(tiny["plus"], tok, ONES))
    ps, rl = U.psnr(on, ref), U.rel_l2(on, ref)
    print("Plus forward %dx%d: PSNR %.2f dB, rel-L2 %.3g" % (hw + (ps, rl)))
    U.record_parity("ip_plus_forward_tiny_%dx%d" % hw, dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert on.shape == ref.shape and torch.isfinite(on).all() and ps >= 55.0 and rl <= 5e-3, (ps, rl)
    pp = U.psnr(on, plain)
    print("Plus forward %dx%d against plain: %.2f dB" % (hw + (pp,)))
    assert pp < 55.0, pp
    native_tok = L.NativeResampler(IR.resampler_of(tiny["plus"]), dim_head=64)(hd)
    assert torch.equal(run(ip_tokens=native_tok), on)
    unet.set_ip_adapter_scale(0.0)
    try:
        assert torch.equal(run(ip_image_embeds=hd), plain)
    finally:
        unet.set_ip_adapter_scale(1.0)
    assert torch.equal(run(), plain)
    assert torch.equal(run(ip_image_embeds=hd), on)


def test_unet_adapter_kinds_refuse_each_other(tiny, lib):
    """[n, E] embeddings on a Plus adapter and [n, T, E] hidden states on a plain adapter raise, in Python and at the C entry; the next
    forward is untouched"""
    import ladi_vton_amd as L
    unet = tiny["mod"]["unet"]
    x, ehs, hidden = IR.unet_case(tiny["ucfg"], 4, 32, 24)
    xd, ed, hd = x.to(U.dev()), ehs.to(U.dev()), hidden.to(U.dev())
    on = unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=hd).sample.float().cpu()
    with pytest.raises(ValueError, match="Plus adapter"):
        unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=hd[:, 0].contiguous())
    with pytest.raises(ValueError, match="Plus adapter"):
        unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=torch.zeros((4, 17, 328), device=U.dev()))
    e = hd[:, 0].contiguous()
    assert lib.ladi_unet_set_ip_context(unet.h, P(e.data_ptr()), 4, stream_ptr()) != 0 and "ladi_unet_set_ip_context_seq" in _lib.last_error()
    assert lib.ladi_unet_set_ip_context_seq(unet.h, P(hd.data_ptr()), 4, 0, stream_ptr()) != 0 and "T >= 1" in _lib.last_error()
    assert torch.equal(unet(xd, T0, encoder_hidden_states=ed, ip_image_embeds=hd).sample.float().cpu(), on)
    with pytest.raises(_lib.NativeError, match="already loaded"):
        unet.load_ip_adapter(tiny["plus"])
    other = L.NativeUNet(tiny["ucfg"], tiny["sd"]["unet"])
    other.load_ip_adapter(R.make_adapter(tiny["ucfg"], 4, 320))
    assert other.ip_adapter_info == (4, 320) and not other.ip_adapter_is_plus
    with pytest.raises(ValueError, match=r"expected \[n, 320\]"):
        other(xd, T0, encoder_hidden_states=ed, ip_image_embeds=hd)
    assert lib.ladi_unet_set_ip_context_seq(other.h, P(hd.data_ptr()), 4, 17, stream_ptr()) != 0 and "plain adapter" in _lib.last_error()
    # a Resampler whose output is not the UNet's cross-attention width, or with a dim_head its width does not divide by: nothing changes
    other.unload_ip_adapter()
    wide = {**{"image_proj." + k: v for k, v in IR.make_resampler(320, 128, 2, 1, 16, 256).items()},
            **{k: v for k, v in tiny["plus"].items() if R.PROC in k}}
    with pytest.raises(_lib.NativeError, match="cross-attention width"):
        other.load_ip_adapter(wide)
    with pytest.raises(_lib.NativeError, match="dim_head 96"):
        other.load_ip_adapter(tiny["plus"], image_proj_dim_head=96)
    assert other.ip_adapter_info is None
    other.load_ip_adapter(tiny["plus"])
    assert other.ip_adapter_is_plus
    assert torch.equal(other(xd, T0, encoder_hidden_states=ed, ip_image_embeds=hd).sample.float().cpu(), on)


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 4


@pytest.fixture(scope="module")
def enc(vision):
    import ladi_vton_amd as L
    return L.NativeCLIPVisionEncoder(VCFG, vision["sd"])


@pytest.fixture(scope="module")
def tiny_plain():
    """a second set of native modules, with a plain adapter whose E is the encoder's projection_dim"""
    t = TT.build()
    t["adapter"] = R.make_adapter(t["ucfg"], 4, 64)
    t["mod"]["unet"].load_ip_adapter(R.to_diffusers(t["adapter"], 2, numbered=True))
    yield t


class _Counting:
    """the encoder behind a counter of its forwards over all-zero pixel_values (the unconditional states)"""

    def __init__(self, enc):
        self.enc, self.zero_forwards, self.forwards = enc, 0, 0
        self.cfg, self.projection_dim = enc.cfg, enc.projection_dim

    def __call__(self, px, output_hidden_states=False):
        self.forwards += 1
        self.zero_forwards += int(not bool(px.any()))
        return self.enc(px, output_hidden_states=output_hidden_states)


def _loop_ref(t, vision, kind, seed=0, pag=0.0):
    key = ("img", kind, seed, pag)
    if key not in t["ref"]:
        adapter = t["plus"] if kind == "plus" else t["adapter"]
        ip = IR.loop_ip(adapter, vision["sd"], VCFG, IR.pictures(2, seed=seed), heads=GEO["heads"])
        a = (t["sd"]["unet"], t["ucfg"], t["sd"]["vae"], t["vcfg"], t["sd"]["emasc"], TT.inputs(t, 2, 64, 48))
        t["ref"][key] = RT.tryon_reference(*a, STEPS, "ddim", ip=ip, pag=(pag, 0.0, ("mid",)), cloth_cond_rate=None)[:2]
    return t["ref"][key]


def _loop(t, pipe, fused=True, graph=True, seed=0, **kw):
    if "ip_adapter_image_embeds" not in kw and not kw.pop("plain", False):
        kw.setdefault("ip_adapter_image", IR.pictures(2, seed=seed).to(U.dev()))
    return TT.call(t, pipe, TT.inputs(t, 2, 64, 48), fused, graph, num_inference_steps=STEPS, **kw)


def _pipe(t, enc):
    pipe = TT.pipe(t)
    pipe.image_encoder = enc
    return pipe


def _arm(t, enc, kind, arm):
    if ("img", kind, arm) not in t["run"]:
        t["run"][("img", kind, arm)] = _loop(t, _pipe(t, enc), fused=arm != "modular", graph=arm == "graph")
    return t["run"][("img", kind, arm)]


@pytest.mark.parametrize("arm", ["graph", "eager", "modular"])
@pytest.mark.parametrize("kind", ["plus", "plain"])
def test_loop_from_a_picture(tiny, tiny_plain, vision, enc, kind, arm):
    """B = 2, 64x48, 4 DDIM steps, `ip_adapter_image=` two random 96x72 pictures: every arm against ref_tryon.tryon_reference (latents >= 40
    dB, image >= 35 dB) fed the reference's own pre-processing, encoder and Resampler; graph == eager bit for bit"""
    t = tiny if kind == "plus" else tiny_plain
    img, lat = _arm(t, enc, kind, arm)
    ref_img, ref_lat = _loop_ref(t, vision, kind)
    p_img, p_lat = TT.assert_close("picture, %s adapter, %s" % (kind, arm), img, lat, ref_img, ref_lat)
    U.record_parity("ip_image_tiny_%s_%s" % (kind, arm), dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    if arm == "eager":
        img_g, lat_g = _arm(t, enc, kind, "graph")
        assert torch.equal(lat, lat_g) and torch.equal(img, img_g)


@pytest.mark.parametrize("kind", ["plus", "plain"])
def test_picture_equals_its_embeddings(tiny, tiny_plain, enc, kind):
    """ip_adapter_image= is ip_adapter_image_embeds=pipe.encode_image(...), bit for bit, as two tensors and as diffusers' [2B] list"""
    t = tiny if kind == "plus" else tiny_plain
    pipe = _pipe(t, enc)
    cond, unc = pipe.encode_image(IR.pictures(2).to(U.dev()))
    assert cond.shape == ((2, 17, 320) if kind == "plus" else (2, 64)) and unc.shape == cond.shape
    if kind == "plain":
        assert not bool(unc.any())
    img, lat = _arm(t, enc, kind, "graph")
    img_e, lat_e = _loop(t, pipe, ip_adapter_image_embeds=cond, negative_ip_adapter_image_embeds=unc)
    assert torch.equal(lat_e, lat) and torch.equal(img_e, img)
    both = torch.cat([unc, cond]) if kind == "plus" else torch.cat([unc, cond])[:, None]
    img_l, lat_l = _loop(t, pipe, ip_adapter_image_embeds=[both])
    assert torch.equal(lat_l, lat) and torch.equal(img_l, img)


def test_loop_lanes_pag_and_no_stale_graph(tiny, vision, enc):
    """Plus adapter: two lanes against one >= 45 dB; pag_scale = 3 against its reference; on one pipeline with use_graph a second picture
    gives other latents that equal their own eager run and meet their own reference; None afterwards is the plain run bit for bit; the
    zero-picture forward of the unconditional states ran once over all of it"""
    counting = _Counting(enc)
    pipe = _pipe(tiny, counting)
    plain = _loop(tiny, pipe, plain=True)
    assert counting.forwards == 0
    img_1, lat_1 = _loop(tiny, pipe)
    assert torch.equal(lat_1, _arm(tiny, enc, "plus", "graph")[1])
    img_2, lat_2 = _loop(tiny, pipe, seed=1)
    TT.assert_close("second picture", img_2, lat_2, *_loop_ref(tiny, vision, "plus", seed=1))
    p = U.psnr(lat_2, lat_1)
    print("second picture against the first: latents %.2f dB" % p)
    assert p < 40.0, p
    img_2e, lat_2e = _loop(tiny, _pipe(tiny, enc), graph=False, seed=1)
    assert torch.equal(lat_2, lat_2e) and torch.equal(img_2, img_2e)
    img_p, lat_p = _loop(tiny, pipe, pag_scale=3.0)
    TT.assert_close("picture with PAG", img_p, lat_p, *_loop_ref(tiny, vision, "plus", pag=3.0))
    after = _loop(tiny, pipe, plain=True)
    assert torch.equal(after[1], plain[1]) and torch.equal(after[0], plain[0])
    assert counting.zero_forwards == 1 and counting.forwards == 3 + 1
    pipe.image_encoder = counting                                   # replacing the encoder drops the cache
    _loop(tiny, pipe)
    assert counting.zero_forwards == 2
    two = _pipe(tiny, enc)
    two.lanes = 2
    _, lat_l = _loop(tiny, two)
    assert two.lib_lanes() == 2
    p = U.psnr(lat_l, lat_1)
    print("picture, two lanes against one: latents %.2f dB" % p)
    assert p >= 45.0, p


def test_picture_misuse_raises_before_any_launch(tiny, tiny_plain, vision, enc, lib):
    """no image_encoder, no adapter, picture and embeddings together, a wrong batch, an encoder without (or with another) projection on a
    plain adapter, hidden states on a plain adapter at the C boundary: each raises with its reason, the encoder never runs, and the next
    plain run on the same handle is the plain run bit for bit"""
    import ladi_vton_amd as L
    pic = IR.pictures(2).to(U.dev())
    counting = _Counting(enc)
    pipe = _pipe(tiny_plain, counting)
    plain = _loop(tiny_plain, pipe, plain=True)
    pipe.image_encoder = None
    with pytest.raises(ValueError, match="image_encoder"):
        _loop(tiny_plain, pipe)
    pipe.image_encoder = counting
    with pytest.raises(ValueError, match="Cannot forward both"):
        _loop(tiny_plain, pipe, ip_adapter_image=pic, ip_adapter_image_embeds=torch.zeros((2, 64), device=U.dev()))
    with pytest.raises(ValueError, match="batch 3"):
        _loop(tiny_plain, pipe, ip_adapter_image=IR.pictures(3).to(U.dev()))
    bare = L.NativeCLIPVisionEncoder(VCFG, {k: v for k, v in vision["sd"].items() if not k.startswith("visual_projection")})
    pipe.image_encoder = bare
    with pytest.raises(ValueError, match="no visual_projection"):
        _loop(tiny_plain, pipe)
    other = dict(vision["sd"])
    other["visual_projection.weight"] = torch.zeros((72, 320))
    pipe.image_encoder = L.NativeCLIPVisionEncoder(VCFG, other)
    with pytest.raises(ValueError, match="projects to 72"):
        _loop(tiny_plain, pipe)
    pipe.image_encoder = counting
    # hidden states on a plain adapter: the pipeline refuses the shape, the library refuses the run
    with pytest.raises(ValueError, match=r"expected \[B, E\]"):
        _loop(tiny_plain, pipe, ip_adapter_image_embeds=torch.zeros((2, 17, 320), device=U.dev()))
    hid = torch.zeros((2, 17, 64), dtype=torch.float16, device=U.dev())
    assert lib.ladi_tryon_set_ip_adapter_seq(pipe._tryon, P(hid.data_ptr()), None, 0) == -1 and "T = 0" in _lib.last_error()
    inp, d = TT.inputs(tiny_plain, 2, 64, 48), U.dev()
    a = (inp["image"], inp["mask_image"].clone(), inp["pose_map"], inp["warped_cloth"], inp["prompt_embeds"].to(d),
         inp["negative_prompt_embeds"].to(d), inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], 64, 48, STEPS, 7.5, 1.0, False, True)
    with pytest.raises(_lib.NativeError, match="plain adapter"):
        pipe._run_fused(*a, ip=(hid, torch.zeros_like(hid)))            # ladi_tryon_set_ip_adapter_seq, then the run: LADI_TRYON_IP_ADAPTER_KIND
    after = _loop(tiny_plain, pipe, plain=True)
    assert torch.equal(after[1], plain[1]) and torch.equal(after[0], plain[0])
    assert counting.forwards == 0
    # no adapter at all
    unet = tiny_plain["mod"]["unet"]
    unet.unload_ip_adapter()
    try:
        with pytest.raises(ValueError, match="needs a loaded IP-Adapter"):
            _loop(tiny_plain, pipe)
    finally:
        unet.load_ip_adapter(tiny_plain["adapter"])
    assert counting.forwards == 0
    # a Plus adapter refuses one embedding per image, in the pipeline and in the library
    pp = _pipe(tiny, counting)
    with pytest.raises(ValueError, match="Plus adapter"):
        _loop(tiny, pp, ip_adapter_image_embeds=torch.zeros((2, 320), device=U.dev()))
    assert counting.forwards == 0
