"""LoRA on the device: the merge kernel element by element against tests/lora_ref.py (guarded buffers, both row maps, padding columns, ranks
1 .. 128, up to eight adapters, the restore path, the non-finite counter), the weight read-back, then the native UNet with adapters against a
twin built from the exported weights (bit-equal forward, oracle parity), no drift / order / restore, the context cache, the fused loop with
its captured graph, the re-packed operands of the fused sub-blocks, and the guard and error paths.  UNET_TINY and 8x8 latents throughout."""
import ctypes
from collections import OrderedDict

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import stream_ptr
from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P
from tests import lora_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ 1. the operator
FILL_W, FILL_B = 3.0, 9.0
SHAPES = {"64x64": (64, 64, 1, False, 1), "64x31x9": (64, 31, 9, False, 1), "128x64geglu": (128, 64, 1, True, 1), "192x128x3blocks": (192, 128, 1, False, 3),
          "256x256x9": (256, 256, 9, False, 1)}
RANKS = {"r1": [1], "r4": [4], "r7": [7], "r128": [128], "r4+r7": [4, 7], "eight": [1, 2, 3, 4, 5, 6, 7, 8]}


def _case(name, ranks, seed):
    """base weight + factors of one operator case, the float64 reference and its limit"""
    rows, cin, taps, geglu, blocks = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    k = int(round(taps ** 0.5))
    shape = (rows, cin, k, k) if taps > 1 else (rows, cin)
    base = (torch.randn(shape, generator=g) * (3.0 / (cin * taps)) ** 0.5).half().float()
    fs = []
    for i, r in enumerate(ranks):
        up = 0.05 * torch.randn((rows, r), generator=g)
        down = 0.05 * torch.randn((r,) + shape[1:], generator=g)
        fs.append((R.fp32_scale([1.0, 0.5, 2.0, -1.0][i % 4], [r, 2 * r, 1.0][i % 3], r), up, down))
    return base, fs


def _launch(lib, gb, gw, cin, taps, row0, rows, half, fs_dev, cnt=None):
    """ladi_op_lora_merge on guarded base / W; fs_dev: [(scale, up device [rows, r], down device [r, taps, cin]), ..] -> rc"""
    n = len(fs_dev)
    Pp = ctypes.c_void_p
    ups, dns = (Pp * 8)(*[f[1].data_ptr() for f in fs_dev]), (Pp * 8)(*[f[2].data_ptr() for f in fs_dev])
    rk, sc = (ctypes.c_int * 8)(*[f[1].shape[1] for f in fs_dev]), (ctypes.c_float * 8)(*[f[0] for f in fs_dev])
    rc = lib.ladi_op_lora_merge(gb.ptr, gw.ptr, gw.ld, cin, R.pad64(cin), taps, row0, rows, half, n, ups, dns, rk, sc,
                                cnt.data_ptr() if cnt is not None else None, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _dev_factors(fs, taps, lo=0, hi=None):
    """factors on the device in the operator's layouts, rows [lo, hi) of up"""
    out = []
    for scale, up, down in fs:
        r, cin = down.shape[0], down.shape[1]
        out.append((scale, up[lo:hi].contiguous().to(U.dev()), down.reshape(r, cin, taps).permute(0, 2, 1).contiguous().to(U.dev())))
    return out


@pytest.mark.parametrize("rk", list(RANKS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_op_merge_within_the_bound(lib, name, rk):
    """ladi_op_lora_merge on guarded buffers (pitch = row + 8 halves, NaN around), the block at row 64 of a larger weight (the 192-row case:
    three 64-row launches at row0 = 0 / 64 / 128, i.e. three members of a concatenated weight).

    The bound.  With u = 2^-24 and every factor value an fp32 number, the kernel computes, per element, s_a = sum_r up[o][r] down[r][t][i] as an
    fmaf chain over ascending r (r_a roundings), d = fmaf(scale_a, s_a, d) over the adapters in call order (one rounding each) and
    float(base) + d (one rounding): the term of adapter a passes through r_a + (A - a + 1) + 1 roundings, at most K + 2 for K the summed rank,
    the base through one.  By the running-error bound of a sum of products (Higham, Accuracy and Stability, eq. 3.7 / 4.4, gamma_n ~ n u) the
    value that is finally rounded to fp16 differs from the exact one by at most
        delta = (K + 4) u (|base| + sum_a |scale_a| sum_r |up| |down|)
    (two units of slack cover gamma_n against n u up to K = 2048).  Rounding to fp16 moves that value by half a spacing at its own magnitude,
    which is at most |ref| + delta:  |got - ref| <= 1/2 ulp16(|ref| + delta) + delta  (lora_ref.merge_limit).  fp16 products of the factors
    would not meet it: the bound assumes fp32 products.

    Also: columns [cin, cin_pad) of the block and every row outside it keep their bits, a second launch is bit-equal, zero adapters and a
    scale of 0 give the base's bits."""
    rows, cin, taps, geglu, blocks = SHAPES[name]
    ranks = RANKS[rk]
    base, fs = _case(name, ranks, 100 * len(name) + sum(ranks))
    row0, total = (0, rows + 64) if blocks > 1 else (64, rows + 128)
    cp = R.pad64(cin)
    gb = U.guarded(R.pack_rows(base, total, row0, geglu, fill=FILL_B), ld=taps * cp + 8)
    w0 = torch.full((total, taps * cp), FILL_W, dtype=torch.float16)
    gw = U.guarded(w0, ld=taps * cp + 8)
    base_bits = _bits(gb.cpu())
    br = rows // blocks
    for b in range(blocks):
        rc = _launch(lib, gb, gw, cin, taps, row0 + b * br, br, br // 2 if geglu else 0, _dev_factors(fs, taps, b * br, (b + 1) * br))
        assert rc == 0, _lib.last_error()
    got_p = gw.cpu()
    ref, mag, K = R.merge_ref(base, fs)
    assert K == sum(ranks)
    got = R.unpack_rows(got_p, rows, cin, taps, row0, geglu)
    ref3, lim = ref.reshape(rows, cin, taps), R.merge_limit(ref, mag, K).reshape(rows, cin, taps)
    err = (got - ref3).abs()
    assert bool(torch.isfinite(got).all())
    worst = float((err / lim).max())
    print("%s %s: worst err / limit %.3f" % (name, rk, worst))
    assert bool((err <= lim).all()), (worst, int((err > lim).sum()))
    assert float((got - base.reshape(rows, cin, taps).double()).abs().max()) > 0            # and something was merged
    # what must keep its bits: the padding columns of the block, every other row, the poison around both buffers, the base
    keep = torch.ones((total, taps, cp), dtype=torch.bool)
    blk = torch.zeros((rows, taps, cp), dtype=torch.bool)
    blk[:, :, :cin] = True
    keep[R.row_map(rows, row0, geglu)] = ~blk
    keep = keep.reshape(total, taps * cp)
    assert torch.equal(_bits(got_p)[keep], _bits(w0)[keep])
    U.assert_untouched(gw, "W"); U.assert_untouched(gb, "base")
    assert torch.equal(_bits(gb.cpu()), base_bits)
    # a second launch: bit-equal
    for b in range(blocks):
        assert _launch(lib, gb, gw, cin, taps, row0 + b * br, br, br // 2 if geglu else 0, _dev_factors(fs, taps, b * br, (b + 1) * br)) == 0
    assert torch.equal(_bits(gw.cpu()), _bits(got_p))
    # scale 0, then zero adapters over a dirtied block: the base's bits
    want = R.unpack_rows(gb.cpu(), rows, cin, taps, row0, geglu)
    for zero in ("scale", "none"):
        gw.view.copy_(w0.to(U.dev()))
        for b in range(blocks):
            f = _dev_factors([(0.0, up, down) for _, up, down in fs], taps, b * br, (b + 1) * br) if zero == "scale" else []
            assert _launch(lib, gb, gw, cin, taps, row0 + b * br, br, br // 2 if geglu else 0, f) == 0
        now = gw.cpu()
        assert torch.equal(R.unpack_rows(now, rows, cin, taps, row0, geglu), want), zero
        assert torch.equal(_bits(now)[keep], _bits(w0)[keep]), zero


def test_op_counts_the_results_that_leave_fp16(lib):
    """base 60000 everywhere, one rank-1 adapter whose delta is up[o] * down[i] = 1 * d_i with d_i from 0 to 7000: the counter receives exactly
    the number of elements fp16(60000 + d) rounds to infinity (65520 and above), over two launches it accumulates, and a null counter is fine"""
    rows, cin = 64, 64
    base = torch.full((rows, cin), 60000.0)
    d = torch.linspace(0.0, 7000.0, cin)
    up, down = torch.ones((rows, 1)), d.reshape(1, cin).clone()
    gb, gw = U.guarded(R.pack_rows(base), ld=72), U.guarded(torch.zeros((rows, cin), dtype=torch.float16), ld=72)
    cnt = torch.zeros(1, dtype=torch.int32, device=U.dev())
    want = int(torch.isinf((base + up @ down).half()).sum())
    assert 0 < want < rows * cin
    fs = _dev_factors([(1.0, up, down)], 1)
    assert _launch(lib, gb, gw, cin, 1, 0, rows, 0, fs, cnt) == 0
    assert int(cnt.item()) == want
    assert int(torch.isinf(gw.cpu()).sum()) == want
    assert _launch(lib, gb, gw, cin, 1, 0, rows, 0, fs, cnt) == 0 and int(cnt.item()) == 2 * want
    assert _launch(lib, gb, gw, cin, 1, 0, rows, 0, fs, None) == 0


# ------------------------------------------------------------------------------------------------------------------ the UNet
T0 = 481
CFG = C.UNET_TINY
WSHAPES = {k[:-len(".weight")]: s for k, s in C.unet_shapes(CFG).items() if k.endswith(".weight") and len(s) >= 2}
XF0 = "down_blocks.0.attentions.0.transformer_blocks.0"
# one module of every target kind (what adapter "b" touches; adapter "a" touches every conv and linear)
KINDS = ["conv_in", "conv_out", "time_embedding.linear_1", "time_embedding.linear_2", "down_blocks.1.resnets.0.conv1", "down_blocks.1.resnets.0.conv2",
         "down_blocks.1.resnets.0.conv_shortcut", "down_blocks.1.resnets.0.time_emb_proj", "up_blocks.3.resnets.2.time_emb_proj",
         "down_blocks.0.downsamplers.0.conv", "up_blocks.1.upsamplers.0.conv", "down_blocks.0.attentions.0.proj_in", XF0 + ".attn1.to_q", XF0 + ".attn1.to_k",
         XF0 + ".attn1.to_v", XF0 + ".attn1.to_out.0", XF0 + ".attn2.to_q", XF0 + ".attn2.to_k", XF0 + ".attn2.to_v", XF0 + ".attn2.to_out.0",
         XF0 + ".ff.net.0.proj", XF0 + ".ff.net.2", "down_blocks.0.attentions.0.proj_out"]


def _inputs(n, seed=7, hw=(8, 8), L_=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 31) + hw, generator=g).half().float()
    ehs = torch.randn((n, L_, CFG["cross_attention_dim"]), generator=g).half().float()
    return x, ehs


def _fwd(unet, x, ehs):
    return unet(x.to(U.dev()), T0, encoder_hidden_states=ehs.to(U.dev())).sample.float().cpu()


def _export(unet):
    return OrderedDict((m + ".weight", unet.export_weight(m + ".weight")) for m in WSHAPES)


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def env():
    import ladi_vton_amd as L
    sd = C.synth_state_dict(C.unet_shapes(CFG), "unet.")
    unet = L.NativeUNet(CFG, sd)
    x2, e2 = _inputs(2)
    plain = _fwd(unet, x2, e2)                       # before any load
    exported0 = _export(unet)
    ad_a = R.make_adapter(11, WSHAPES, {m: (4 if i % 2 else 7) for i, m in enumerate(WSHAPES)}, conv_up_4d=True)
    ad_b = R.make_adapter(12, WSHAPES, {m: (7 if i % 2 else 4) for i, m in enumerate(KINDS)}, alpha=2.0)
    unet.load_lora_adapter(ad_a, "a")
    unet.load_lora_adapter(ad_b, "b")
    yield dict(L=L, sd=sd, unet=unet, plain=plain, exported0=exported0, a=ad_a, b=ad_b, x2=x2, e2=e2, twin={})
    unet.set_adapters([])


@pytest.fixture(autouse=True)
def _plain_between_tests(request):
    yield
    if "env" in request.fixturenames:
        request.getfixturevalue("env")["unet"].set_adapters([])


def _twin(env):
    """the UNet with adapter "a" active, its export, and a second UNet built from that export (norms and biases from the original)"""
    if not env["twin"]:
        env["unet"].set_adapters(["a"])
        exp = env["unet"].export_state_dict(env["sd"])
        env["twin"] = dict(exp=exp, unet=env["L"].NativeUNet(CFG, exp))
    env["unet"].set_adapters(["a"])
    return env["twin"]


def test_export_round_trip(env):
    """no adapter active: the read-back equals the synthetic state dict exactly for every conv / linear .weight key (and the table has them all)"""
    assert env["unet"].list_adapters() == ["a", "b"] and env["unet"].active_adapters == []
    keys = [k for k, s in C.unet_shapes(CFG).items() if k.endswith(".weight") and len(s) >= 2]
    assert list(env["exported0"]) == keys and len(keys) == 282
    for k in keys:
        assert env["exported0"][k].shape == env["sd"][k].shape and torch.equal(env["exported0"][k], env["sd"][k]), k
    assert env["unet"].lib.ladi_unet_export_weight(env["unet"].h, b"conv_norm_out.weight", None, 0) == -1 and "conv / linear" in _lib.last_error()
    buf = torch.empty(4)
    assert env["unet"].lib.ladi_unet_export_weight(env["unet"].h, b"conv_in.weight", buf.data_ptr(), 4) == -1 and "do not fit" in _lib.last_error()


def test_merged_twin(env):
    """adapter "a": a factor pair on every conv and linear, ranks 4 and 7 alternating (conv up factors 4-D).  The exported weights stay
    within the bound of test_op_merge_within_the_bound against lora_ref; a second NativeUNet built from the export gives a bit-equal forward
    (n = 2 and n = 4); the oracle forward on the exported weights meets test_unet_forward_tiny's bound (PSNR >= 55 dB, rel-L2 <= 5e-3)"""
    tw = _twin(env)
    assert env["unet"].active_adapters == [("a", 1.0)]
    refs = R.merged_state_dict(env["sd"], [(env["a"], 1.0)])
    assert len(refs) == 282
    worst = 0.0
    for k, (ref, mag, K) in refs.items():
        lim = R.merge_limit(ref, mag, K)
        err = (tw["exp"][k].double() - ref).abs()
        assert bool((err <= lim).all()), (k, float((err / lim).max()))
        worst = max(worst, float((err / lim).max()))
        assert not torch.equal(tw["exp"][k], env["sd"][k]), k
    print("export against the float64 merge: worst err / limit %.3f" % worst)
    for k in env["sd"]:
        if k not in refs:
            assert torch.equal(tw["exp"][k], env["sd"][k]), k
    for n in (2, 4):
        x, ehs = _inputs(n, seed=20 + n)
        got, twin = _fwd(env["unet"], x, ehs), _fwd(tw["unet"], x, ehs)
        assert torch.isfinite(got).all() and torch.equal(got, twin), n
        if n == 2:
            ref = M.unet_forward(tw["exp"], CFG, x, T0, ehs)
            ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
            print("merged forward against the oracle on the exported weights: PSNR %.2f dB, rel-L2 %.3g" % (ps, rl))
            assert ps >= 55.0 and rl <= 5e-3, (ps, rl)
    assert U.psnr(_fwd(env["unet"], env["x2"], env["e2"]), env["plain"]) < 55.0             # and it is another function than the plain UNet


def test_no_drift_order_restore(env):
    unet = env["unet"]
    unet.set_adapters(["a"], [1.0])
    unet.set_adapters(["a", "b"], [0.5, 2.0])
    both = _export(unet)
    unet.set_adapters(["a"], [0.5])
    assert unet.active_adapters == [("a", 0.5)]
    walked = _export(unet)
    fresh = env["L"].NativeUNet(CFG, env["sd"])
    fresh.load_lora_adapter(env["a"], "a")
    fresh.load_lora_adapter(env["b"], "b")
    fresh.set_adapters(["a"], [0.5])
    assert _same(walked, _export(fresh))
    # two adapters: within the bound, and the order is the call order
    refs = R.merged_state_dict(env["sd"], [(env["a"], 0.5), (env["b"], 2.0)])
    for m in KINDS:
        ref, mag, K = refs[m + ".weight"]
        assert K in (8, 11, 14) and bool(((both[m + ".weight"].double() - ref).abs() <= R.merge_limit(ref, mag, K)).all()), m
    fresh.set_adapters(["b", "a"], [2.0, 0.5])
    assert fresh.active_adapters == [("b", 2.0), ("a", 0.5)]
    # restore: [] and disable_lora() give the original bits and the original forward; enable_lora() brings the set back
    unet.set_adapters([])
    assert _same(_export(unet), env["exported0"]) and torch.equal(_fwd(unet, env["x2"], env["e2"]), env["plain"])
    unet.set_adapters(["a", "b"], [0.5, 2.0])
    unet.disable_lora()
    assert unet.active_adapters == [] and _same(_export(unet), env["exported0"]) and torch.equal(_fwd(unet, env["x2"], env["e2"]), env["plain"])
    unet.enable_lora()
    assert unet.active_adapters == [("a", 0.5), ("b", 2.0)] and _same(_export(unet), both)


def test_context_is_dropped_and_rebuilt(env):
    unet, lib = env["unet"], env["unet"].lib
    tw = _twin(env)
    unet.set_adapters([])
    x, ehs = _inputs(2, seed=31)
    xd, ed = x.to(U.dev()), ehs.to(U.dev())
    before = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    unet.set_adapters(["a"])
    out = torch.empty((2, 4, 8, 8), dtype=torch.float32, device=U.dev())
    rc = lib.ladi_unet_forward(unet.h, xd.data_ptr(), _lib.F32, 2, 8, 8, float(T0), out.data_ptr(), _lib.F32, stream_ptr())
    assert rc != 0 and "set_context" in _lib.last_error()
    got = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()          # the SAME tensor object: the K/V cache is rebuilt all the same
    twin = tw["unet"](xd, T0, encoder_hidden_states=ed).sample.float().cpu()
    assert torch.equal(got, twin) and not torch.equal(got, before)


# ------------------------------------------------------------------------------------------------------------------ fused loop
H_IMG, W_IMG, STEPS = 64, 48, 3


def _pipe(L, unet, mods):
    return L.StableDiffusionTryOnePipeline(vae=mods["vae"], text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(),
                                           emasc=mods["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _run(pipe, inp, graph=True):
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H_IMG, width=W_IMG, num_inference_steps=STEPS,
               guidance_scale=7.5, output_type="np", fused=True, use_graph=graph,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def test_fused_loop_and_graph(env):
    """one pipeline, use_graph: plain -> load_lora_weights (loads and activates) -> disable.  Runs 1 and 3 are bit-equal; run 2 equals the same
    call on a fresh pipeline around the twin UNet and the run without the graph: the captured graph reads the merged weights in place"""
    L = env["L"]
    vcfg = C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    mods = dict(vae=L.NativeVAE(vcfg, C.synth_state_dict(C.vae_shapes(vcfg), "vae.")),
                emasc=L.NativeEMASC(ecfg, C.synth_state_dict(C.emasc_shapes(ecfg), "emasc.")))
    inp = P.synthetic_inputs(1, H_IMG, W_IMG, L=8, D=CFG["cross_attention_dim"])
    for k in ("prompt_embeds", "negative_prompt_embeds"):
        inp[k] = inp[k].half().float()
    tw = _twin(env)
    env["unet"].set_adapters([])
    pipe = _pipe(L, env["unet"], mods)
    img_1, lat_1 = _run(pipe, inp)
    ad_c = R.make_adapter(11, WSHAPES, {m: (4 if i % 2 else 7) for i, m in enumerate(WSHAPES)})     # adapter "a" again, under another name
    pipe.load_lora_weights(ad_c, adapter_name="c")
    assert pipe.get_active_adapters() == ["c"] and pipe.get_list_adapters() == {"unet": ["a", "b", "c"]}
    img_2, lat_2 = _run(pipe, inp)
    img_e, lat_e = _run(pipe, inp, graph=False)
    pipe.disable_lora()
    img_3, lat_3 = _run(pipe, inp)
    assert torch.equal(lat_3, lat_1) and torch.equal(img_3, img_1)
    # loading while disabled: the set that was put aside counts as active, so it comes back together with the new adapter
    m = XF0 + ".attn1.to_q"
    pipe.load_lora_weights({m + ".lora_A.weight": torch.zeros((2, WSHAPES[m][1])), m + ".lora_B.weight": torch.zeros((WSHAPES[m][0], 2))}, adapter_name="d")
    assert env["unet"].active_adapters == [("c", 1.0), ("d", 1.0)]
    pipe.set_adapters([])
    pipe.delete_adapters(["c", "d"])
    assert pipe.get_list_adapters() == {"unet": ["a", "b"]}
    assert torch.isfinite(lat_2).all() and not torch.equal(lat_2, lat_1)
    assert torch.equal(lat_2, lat_e) and torch.equal(img_2, img_e)
    img_t, lat_t = _run(_pipe(L, tw["unet"], mods), inp)
    assert torch.equal(lat_2, lat_t) and torch.equal(img_2, img_t)


def _igemm_log_of(lib, fn):
    """the implicit-GEMM launches fn() makes, as launch-log records"""
    from tests import tuned_cases
    lib.ladi_igemm_launch_log(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.ladi_igemm_launch_log(0)
    return out, tuned_cases.read_log(lib)


def test_fused_sub_block_operands_are_repacked(monkeypatch, lib):
    """LADI_XF_FUSE=2: level 0 (C = 320, 5 heads, 128 tokens) runs attn2 and the feed-forward from re-packed copies of attn2.to_out.0 and
    ff.net.2.  An adapter on exactly those two gives a forward bit-equal to its twin built under the same setting (and not the plain one).
    That the fused route is the one in use is read from the launch log: ff.net.2 of level 0 is the only implicit GEMM of this UNet with
    K = 1280 and Q = 320; a UNet built under LADI_XF_FUSE=0 launches it, the fused one never does."""
    import ladi_vton_amd as L
    cfg = dict(CFG, block_out_channels=(320, 64, 64, 64), num_heads=(5, 1, 1, 1), cross_attention_dim=128)
    sd = C.synth_state_dict(C.unet_shapes(cfg), "unet.")
    shapes = {k[:-len(".weight")]: s for k, s in C.unet_shapes(cfg).items()}
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 31, 16, 8), generator=g).half().float()
    ehs = torch.randn((2, 8, 128), generator=g).half().float()
    is_ff2 = lambda r: r["K"] == 1280 and r["Q"] == 320
    monkeypatch.setenv("LADI_XF_FUSE", "0")
    unfused = L.NativeUNet(cfg, sd)
    _, log0 = _igemm_log_of(lib, lambda: _fwd(unfused, x, ehs))
    print("unfused: ff.net.2 launches", sum(r["n"] for r in log0 if is_ff2(r)))
    assert sum(r["n"] for r in log0 if is_ff2(r)) >= 1
    del unfused
    monkeypatch.setenv("LADI_XF_FUSE", "2")
    unet = L.NativeUNet(cfg, sd)
    plain, log2 = _igemm_log_of(lib, lambda: _fwd(unet, x, ehs))
    assert log2 and not [r for r in log2 if is_ff2(r)]                  # the fused feed-forward ran instead
    b = "down_blocks.0.attentions.1.transformer_blocks.0"
    ad = R.make_adapter(3, shapes, {b + ".attn2.to_out.0": 4, b + ".ff.net.2": 7})
    unet.load_lora_adapter(ad, "f")
    unet.set_adapters(["f"])
    got, log3 = _igemm_log_of(lib, lambda: _fwd(unet, x, ehs))
    assert not [r for r in log3 if is_ff2(r)]
    twin = L.NativeUNet(cfg, unet.export_state_dict(sd))
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    assert torch.equal(got, _fwd(twin, x, ehs))
    unet.set_adapters([])
    assert torch.equal(_fwd(unet, x, ehs), plain)


# ------------------------------------------------------------------------------------------------------------------ guard and errors
def test_guard_and_errors(env):
    unet, NE = env["unet"], _lib.NativeError
    unet.set_adapters(["a"], [0.75])
    before = _export(unet)
    m = XF0 + ".attn1.to_v"
    rows, cin = WSHAPES[m]
    big = {m + ".lora_down.weight": torch.full((1, cin), 300.0), m + ".lora_up.weight": torch.full((rows, 1), 300.0)}
    unet.load_lora_adapter(big, "big")
    with pytest.raises(NE, match=m.replace(".", r"\.")):
        unet.set_adapters(["a", "big"])
    assert unet.active_adapters == [("a", 0.75)] and _same(_export(unet), before)
    x, ehs = _inputs(2, seed=41)
    assert torch.isfinite(_fwd(unet, x, ehs)).all()
    unet.delete_adapters("big")
    ok = {m + ".lora_down.weight": torch.zeros((4, cin)), m + ".lora_up.weight": torch.zeros((rows, 4))}
    with pytest.raises(ValueError):                                    # unknown module: refused by the normaliser ..
        unet.load_lora_adapter({"down_blocks.0.nope.lora_A.weight": ok[m + ".lora_down.weight"], "down_blocks.0.nope.lora_B.weight": ok[m + ".lora_up.weight"]}, "x")
    from ladi_vton_amd.modules import _Weights
    with _Weights({"down_blocks.0.nope.lora_down.weight": torch.zeros((4, cin)), "down_blocks.0.nope.lora_up.weight": torch.zeros((rows, 4))}) as w:
        assert unet.lib.ladi_unet_lora_load(unet.h, b"x", w.h) != 0 and "unknown module" in _lib.last_error()      # .. and by the library
    for bad, pat in ((dict(ok, **{m + ".lora_down.weight": torch.zeros((4, cin + 1))}), "does not fit"),
                     (dict(ok, **{m + ".lora_up.weight": torch.zeros((rows + 1, 4))}), "does not fit"),
                     ({m + ".lora_down.weight": torch.zeros((257, cin)), m + ".lora_up.weight": torch.zeros((rows, 257))}, "rank 257"),
                     ({m + ".lora_down.weight": torch.zeros((0, cin)), m + ".lora_up.weight": torch.zeros((rows, 0))}, None)):
        with pytest.raises(NE, match=pat):
            unet.load_lora_adapter(bad, "x")
    with pytest.raises(NE, match="already loaded"):
        unet.load_lora_adapter(ok, "a")
    with pytest.raises(NE, match="is active"):
        unet.delete_adapters("a")
    with pytest.raises(NE, match="no adapter named"):
        unet.set_adapters(["a", "nobody"])
    with pytest.raises(NE, match="twice"):
        unet.set_adapters(["a", "a"])
    assert unet.list_adapters() == ["a", "b"]
    for i in range(6):
        unet.load_lora_adapter(ok, "n%d" % i)
    with pytest.raises(NE, match="at most 8"):
        unet.load_lora_adapter(ok, "ninth")
    assert unet.list_adapters() == ["a", "b"] + ["n%d" % i for i in range(6)]
    unet.delete_adapters(["n%d" % i for i in range(6)])
    assert unet.list_adapters() == ["a", "b"] and unet.active_adapters == [("a", 0.75)] and _same(_export(unet), before)
