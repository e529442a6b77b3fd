"""Token merging on the device: the four operators (csrc/tome.hip) on strided views in poisoned buffers against tests/tome_ref.py, the
native UNet's forward with the device's own plans forced into the reference forward, the wiring of the metric, then the tiny model end to
end (fused hipGraph, fused eager, modular; feature cache, PAG on the mid block, LCM, lanes), the graph key and the misuse."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr, stream_ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import ref_tryon as RT
from tests import ref_unet as RU
from tests import tome_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

SHAPES = [(2, 6, 8, 64), (1, 5, 7, 128), (2, 12, 16, 640), (1, 48, 64, 320)]      # n, h, w, C
GUARD = -0x5A5A5A5B


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(U.cpu_quota_threads())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _idev(v):
    return torch.as_tensor(v, dtype=torch.int32).contiguous().to(U.dev())


class IBuf:
    """an int32 / float32 device output of `count` words between two guard zones of 64 words"""

    def __init__(self, count, dtype=torch.int32):
        self.buf = torch.full((count + 128,), GUARD, dtype=torch.int32, device=U.dev())
        self.count, self.dtype = count, dtype
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 256)

    def cpu(self):
        return self.buf[64:64 + self.count].view(self.dtype).cpu()

    def assert_guards(self, what):
        b = self.buf.cpu()
        assert bool((b[:64] == GUARD).all()) and bool((b[64 + self.count:] == GUARD).all()), what + ": wrote outside its output"


def _geometry(h, w, use_rand=False, seed=0):
    sp, dp = R.tables(h, w, 2, 2, use_rand, seed)
    return sp, dp, h * w, len(sp), len(dp)


# ------------------------------------------------------------------------------------------------------------------ match
def _match_data(n, T, Cc, sp, dp, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "integer":
        # rows of k^2 entries +-1 (k = 1, 2, 4): norms 1, 2, 4, so normalised rows, products and sums are exact in fp16 / fp32; not symmetric
        x = torch.zeros((n, T, Cc))
        for s in range(n):
            for p in range(T):
                k = (1, 4, 16)[int(torch.randint(0, 3, (1,), generator=g))]
                cols = torch.randperm(32, generator=g)[:k]          # a narrow band: many overlaps, many exact ties
                x[s, p, cols] = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
        return x.half()
    x = (torch.randn((n, T, Cc), generator=g) * 1.5 + 0.3).half()
    if kind == "special":
        x[0, dp[1]] = x[0, dp[4]]                 # an exactly duplicated dst row, and a src row that is a copy of both: the lower j wins
        x[0, sp[3]] = x[0, dp[4]]
        x[-1, sp[5]] = 0                          # an all-zero src row scores 0
    return x


def _run_match(lib, x, n, T, Cc, sp, dp):
    Ns, Nd = len(sp), len(dp)
    gx = U.guarded(x.reshape(n * T, Cc), ld=Cc + 8)
    ws = torch.full((lib.ladi_op_tome_match_workspace_bytes(n, Ns, Nd, Cc) // 2,), float("nan"), dtype=torch.float16, device=U.dev())
    sc, nd = IBuf(n * Ns, torch.float32), IBuf(n * Ns)
    dsp, ddp = _idev(sp), _idev(dp)
    rc = lib.ladi_op_tome_match(ctypes.c_void_p(gx.ptr), gx.ld, T * gx.ld, ptr(dsp), ptr(ddp), n, T, Ns, Nd, Cc, ptr(ws), sc.ptr, nd.ptr, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert torch.equal(_bits(gx.cpu()), _bits(x.reshape(n * T, Cc)))
    U.assert_untouched(gx, "tome_match x")
    sc.assert_guards("score"), nd.assert_guards("node")
    assert torch.equal(dsp.cpu(), torch.as_tensor(sp, dtype=torch.int32)) and torch.equal(ddp.cpu(), torch.as_tensor(dp, dtype=torch.int32))
    return sc.cpu().view(n, Ns), nd.cpu().view(n, Ns).long()


@pytest.mark.parametrize("kind", ["random", "special"])
@pytest.mark.parametrize("n,h,w,Cc", SHAPES)
def test_match_op(lib, n, h, w, Cc, kind):
    """score and node against float64 cosine scores of the same fp16 input: S_ref[i, node[i]] >= max_j S_ref[i, j] - delta and
    |score[i] - S_ref[i, node[i]]| <= delta, delta = 2^-9 (two fp16 roundings of unit vectors perturb a dot product by at most 2^-10, fp32
    accumulation over C <= 640 adds less than 2^-13; delta is twice that)"""
    sp, dp, T, Ns, Nd = _geometry(h, w)
    x = _match_data(n, T, Cc, sp, dp, kind, 3 * h + Cc)
    score, node = _run_match(lib, x, n, T, Cc, sp, dp)
    delta = 2.0 ** -9
    assert int(node.min()) >= 0 and int(node.max()) < Nd
    for s in range(n):
        S = R.scores(x[s], sp, dp, torch.float64)
        at = S.gather(1, node[s][:, None])[:, 0]
        worst_gap = float((S.max(dim=1).values - at).max())
        worst_err = float((score[s].double() - at).abs().max())
        print("tome_match %s n=%d %dx%d C=%d sample %d: argmax gap %.3g, score error %.3g (delta %.3g)" % (kind, n, h, w, Cc, s, worst_gap, worst_err, delta))
        assert worst_gap <= delta and worst_err <= delta, (worst_gap, worst_err)
    if kind == "special":
        assert int(node[0, 3]) == 1 and abs(float(score[0, 3]) - 1.0) <= delta        # dst 1 and dst 4 are equal: the lower wins
        assert float(score[-1, 5]) == 0.0


@pytest.mark.parametrize("n,h,w,Cc", SHAPES)
def test_match_op_integer_data_is_exact(lib, n, h, w, Cc):
    """integer-valued, non-symmetric rows whose norms are 1, 2 or 4: every product and sum is exact, so score and node (the lowest dst that
    reaches the maximum) equal the float64 reference exactly -- the check of the MFMA fragment maps"""
    sp, dp, T, Ns, Nd = _geometry(h, w)
    x = _match_data(n, T, Cc, sp, dp, "integer", h + w)
    score, node = _run_match(lib, x, n, T, Cc, sp, dp)
    for s in range(n):
        S = R.scores(x[s], sp, dp, torch.float64)
        rs, rn = R.match(S)
        assert not torch.equal(S[:min(Ns, Nd), :min(Ns, Nd)], S[:min(Ns, Nd), :min(Ns, Nd)].T)
        assert torch.equal(score[s].double(), rs) and torch.equal(node[s], rn)


def test_match_op_refusals(lib):
    sp, dp, T, Ns, Nd = _geometry(6, 8)
    x = torch.zeros((T, 64), dtype=torch.float16, device=U.dev())
    ws = torch.zeros(1 << 16, dtype=torch.float16, device=U.dev())
    sc, nd, dsp, ddp = IBuf(Ns, torch.float32), IBuf(Ns), _idev(sp), _idev(dp)
    run = lambda C_, ld, T_=T: lib.ladi_op_tome_match(ptr(x), ld, T * ld, ptr(dsp), ptr(ddp), 1, T_, Ns, Nd, C_, ptr(ws), sc.ptr, nd.ptr, stream_ptr())
    assert run(48, 64) != 0 and "channel count" in _lib.last_error()
    assert run(1024, 1024) != 0 and "channel count" in _lib.last_error()
    assert run(64, 32) != 0 and "stride" in _lib.last_error()
    assert run(64, 64, T + 1) != 0 and "count" in _lib.last_error()
    assert lib.ladi_op_tome_match(None, 64, T * 64, ptr(dsp), ptr(ddp), 1, T, Ns, Nd, 64, ptr(ws), sc.ptr, nd.ptr, stream_ptr()) != 0
    torch.cuda.synchronize()
    sc.assert_guards("score"), nd.assert_guards("node")
    assert bool((sc.buf == GUARD).all()) and bool((nd.buf == GUARD).all())


# ------------------------------------------------------------------------------------------------------------------ plan
def _plan_layout(flat, Ns, Nd, r):
    """the sections of one sample's plan buffer"""
    return flat[:Nd + 1].tolist(), flat[Nd + 1:Nd + 1 + Ns - r].tolist(), flat[Nd + 1 + Ns - r:Nd + 1 + Ns].tolist()


def _plan_ints(p, Ns, Nd):
    """a reference plan in the plan buffer's layout (the scratch section zero)"""
    off, src = [0], []
    for seg in p["segs"]:
        src += seg
        off.append(len(src))
    return off + p["unm"] + src + [0] * p["r"]


@pytest.mark.parametrize("which", ["one", "half", "all", "all_but_one"])
@pytest.mark.parametrize("n,h,w,Cc", SHAPES)
def test_plan_op(lib, n, h, w, Cc, which):
    """supplied scores (four distinct values, so exact ties, some across the r-th place, -0 against +0 and one NaN) and nodes: out_row and
    the plan's sections equal the reference's exactly"""
    sp, dp, T, Ns, Nd = _geometry(h, w, True, 5)
    r = dict(one=1, half=int(T / 2), all=Ns, all_but_one=Ns - 1)[which]
    g = torch.Generator().manual_seed(T + r)
    score = torch.tensor([0.25, 0.5, 0.0, -0.5])[torch.randint(0, 4, (n, Ns), generator=g)]
    score[:, 2] = float("nan")
    score[:, 4], score[:, 7] = -0.0, 0.0
    node = torch.randint(0, Nd, (n, Ns), generator=g)
    ps = lib.ladi_op_tome_plan_ints(Ns, Nd, r)
    assert ps == Nd + 1 + Ns + r
    dsc, dnd, dsp, ddp = score.to(U.dev()), _idev(node), _idev(sp), _idev(dp)
    orow, plan = IBuf(n * T), IBuf(n * ps)
    rc = lib.ladi_op_tome_plan(ptr(dsc), ptr(dnd), ptr(dsp), ptr(ddp), n, T, Ns, Nd, r, orow.ptr, plan.ptr, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    orow.assert_guards("out_row"), plan.assert_guards("plan")
    assert torch.equal(_idev(node).cpu(), dnd.cpu()) and torch.equal(dsc.cpu().view(torch.int32), score.view(torch.int32))
    got_row, got_plan = orow.cpu().view(n, T).long(), plan.cpu().view(n, ps)
    for s in range(n):
        ref = R.plan(score[s], node[s], sp, dp, r)
        assert torch.equal(got_row[s], ref["out_row"]), (which, s)
        off, unm, src = _plan_layout(got_plan[s], Ns, Nd, r)
        want = _plan_ints(ref, Ns, Nd)
        assert off == want[:Nd + 1] and unm == ref["unm"] and src == want[Nd + 1 + Ns - r:Nd + 1 + Ns], (which, s)


def test_plan_op_refusals(lib):
    sp, dp, T, Ns, Nd = _geometry(6, 8)
    sc, nd, dsp, ddp = torch.zeros(Ns, device=U.dev()), _idev([0] * Ns), _idev(sp), _idev(dp)
    orow, plan = IBuf(T), IBuf(2 * T + 8)
    for r in (0, Ns + 1, -1):
        assert lib.ladi_op_tome_plan(ptr(sc), ptr(nd), ptr(dsp), ptr(ddp), 1, T, Ns, Nd, r, orow.ptr, plan.ptr, stream_ptr()) != 0
        assert "count" in _lib.last_error()
    assert lib.ladi_op_tome_plan(ptr(sc), ptr(nd), ptr(dsp), ptr(ddp), 1, 3 * 5000, 2 * 5000, 5000, 4, orow.ptr, plan.ptr, stream_ptr()) != 0
    assert "4096" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((orow.buf == GUARD).all()) and bool((plan.buf == GUARD).all())


# ------------------------------------------------------------------------------------------------------------------ merge / unmerge
def _supplied_plan(sp, dp, seed, r):
    """a plan that no matching produced: r merged src, as many as possible (more than 64 where there are that many) into dst 1, the rest
    spread over every third dst, so some dst have none"""
    Ns, Nd = len(sp), len(dp)
    g = torch.Generator().manual_seed(seed)
    merged = torch.zeros(Ns, dtype=torch.bool)
    merged[torch.randperm(Ns, generator=g)[:r]] = True
    node = torch.randint(0, (Nd + 2) // 3, (Ns,), generator=g) * 3
    node = node.clamp_max(Nd - 1)
    big = merged.nonzero()[:, 0][:min(70, r)]
    node[big] = 1
    return R.make_plan(merged, node, sp, dp)


@pytest.mark.parametrize("n,h,w,Cc", SHAPES)
def test_merge_op(lib, n, h, w, Cc):
    """a supplied plan (one dst with more than 64 sources where the shape has them, dst with none): against the float64 mean within
    |err| <= 2^-10 |ref| + 2^-24 (one fp16 rounding of an fp32 mean of fp16 values); two launches are bit-equal"""
    sp, dp, T, Ns, Nd = _geometry(h, w)
    r = int(0.6 * T) if int(0.6 * T) < Ns else Ns - 1
    g = torch.Generator().manual_seed(T + Cc)
    x = (torch.randn((n, T, Cc), generator=g) * 2).half()
    plans = [_supplied_plan(sp, dp, 10 * s + T, r) for s in range(n)]
    if Ns > 100:
        assert max(len(s) for s in plans[0]["segs"]) > 64
    assert min(len(s) for s in plans[0]["segs"]) == 0
    ps = lib.ladi_op_tome_plan_ints(Ns, Nd, r)
    dplan = _idev([v for p in plans for v in _plan_ints(p, Ns, Nd)])
    gx, ddp = U.guarded(x.reshape(n * T, Cc), ld=Cc + 8), _idev(dp)
    Tm = T - r
    outs = []
    for _ in range(2):
        gy = U.guarded_out(n * Tm, Cc, ld=Cc + 16)
        rc = lib.ladi_op_tome_merge(ctypes.c_void_p(gx.ptr), gx.ld, T * gx.ld, ptr(ddp), ptr(dplan), n, T, Ns, Nd, r, Cc,
                                    ctypes.c_void_p(gy.ptr), gy.ld, Tm * gy.ld, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        U.assert_untouched(gy, "tome_merge y")
        outs.append(gy.cpu().view(n, Tm, Cc))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(_bits(gx.cpu()), _bits(x.reshape(n * T, Cc)))
    U.assert_untouched(gx, "tome_merge x")
    assert dplan.shape[0] == n * ps
    for s in range(n):
        ref = R.merge(x[s], plans[s], torch.float64)
        err = (outs[0][s].double() - ref).abs()
        bound = 2.0 ** -10 * ref.abs() + 2.0 ** -24
        print("tome_merge n=%d %dx%d C=%d sample %d: max err / bound %.3f" % (n, h, w, Cc, s, float((err / bound).max())))
        assert torch.isfinite(outs[0][s]).all() and bool((err <= bound).all())
        Nu = plans[s]["Nu"]
        assert torch.equal(_bits(outs[0][s][:Nu]), _bits(x[s][plans[s]["unm"]]))          # unmerged rows are copies


@pytest.mark.parametrize("n,h,w,Cc", SHAPES)
def test_unmerge_add_op(lib, n, h, w, Cc):
    """bit-equal to (y.float()[out_row] + res.float()).half(); nothing outside the output view changes, the inputs are read only"""
    sp, dp, T, Ns, Nd = _geometry(h, w)
    r = int(T / 2)
    Tm = T - r
    g = torch.Generator().manual_seed(T * Cc)
    y = (torch.randn((n, Tm, Cc), generator=g) * 3).half()
    res = (torch.randn((n, T, Cc), generator=g) * 3).half()
    rows = torch.stack([_supplied_plan(sp, dp, s + T, r)["out_row"] for s in range(n)])
    gy, gr = U.guarded(y.reshape(n * Tm, Cc), ld=Cc + 8), U.guarded(res.reshape(n * T, Cc), ld=Cc + 24)
    go = U.guarded_out(n * T, Cc, ld=Cc + 16)
    drow = _idev(rows)
    rc = lib.ladi_op_tome_unmerge_add(ctypes.c_void_p(gy.ptr), gy.ld, Tm * gy.ld, ctypes.c_void_p(gr.ptr), gr.ld, T * gr.ld, ptr(drow), n, T, Tm, Cc,
                                      ctypes.c_void_p(go.ptr), go.ld, T * go.ld, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    want = torch.stack([(y[s].float()[rows[s]] + res[s].float()).half() for s in range(n)])
    assert torch.equal(_bits(go.cpu().view(n, T, Cc)), _bits(want))
    for gg, what, src in ((gy, "y", y), (gr, "res", res)):
        U.assert_untouched(gg, "tome_unmerge_add " + what)
        assert torch.equal(_bits(gg.cpu()), _bits(src.reshape(-1, Cc)))
    U.assert_untouched(go, "tome_unmerge_add out")
    assert lib.ladi_op_tome_unmerge_add(ctypes.c_void_p(gy.ptr), gy.ld, Tm * gy.ld, ctypes.c_void_p(gr.ptr), gr.ld, T * gr.ld, ptr(drow), n, T, Tm, 12,
                                        ctypes.c_void_p(go.ptr), go.ld, T * go.ld, stream_ptr()) != 0 and "channel count" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------ the UNet forward
T0 = 481
REL_L2, PSNR_DB = 5e-3, 55.0          # the forward comparison of tests/test_gpu_pag.py (test_forward_vs_reference)
LAT_DB, IMG_DB = 40.0, 35.0           # its end-to-end thresholds (_assert_close)


@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    yield dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, fwd={})
    mods["unet"].remove_token_merging()
    if mods["unet"].ip_adapter_info is not None:            # loaded by _adapter for the +ip cases
        mods["unet"].unload_ip_adapter()


@pytest.fixture(autouse=True)
def _off_between_tests(request):
    """token merging and the PAG layers are sticky in the native UNet the tests of this module share"""
    yield
    if "tiny" in request.fixturenames:
        u = request.getfixturevalue("tiny")["mod"]["unet"]
        u.remove_token_merging()
        u.set_pag_applied_layers("mid")
        if u.ip_adapter_info is not None:
            u.set_ip_adapter_scale(1.0)


def _fwd_inputs(tiny, hw, seed=11):
    key = (hw, seed)
    if key not in tiny["fwd"]:
        g = torch.Generator().manual_seed(seed + hw[0])
        x = torch.randn((2, 31) + hw, generator=g).half().float()
        ehs = torch.randn((2, 8, tiny["ucfg"]["cross_attention_dim"]), generator=g).half().float()
        tiny["fwd"][key] = (x, ehs, x.to(U.dev()), ehs.to(U.dev()))
    return tiny["fwd"][key]


IP_SCALES = [1.0] * 16
IP_SCALES[1] = 0.0                    # down_blocks.0.attentions.1: a block that merges and skips the image term


def _adapter(tiny):
    """the IP-Adapter of tests/ip_adapter_ref.py, loaded once into the UNet the module shares (without an image context the forward is the
    plain one), with IP_SCALES set -> (sd_ip, embeds [2, E], tokens [2, N, cross_dim])"""
    from tests import ip_adapter_ref as IR
    unet = tiny["mod"]["unet"]
    if "ip" not in tiny:
        sd_ip = IR.make_adapter(tiny["ucfg"])
        unet.load_ip_adapter(dict(sd_ip))
        emb = torch.randn((2, 64), generator=torch.Generator().manual_seed(77)).half().float()
        tiny["ip"] = (sd_ip, emb, IR.image_proj(sd_ip, emb))
    assert _lib.load().ladi_unet_set_ip_scale(unet.h, (ctypes.c_float * 16)(*IP_SCALES), 16) == 0, _lib.last_error()
    return tiny["ip"]


def _device_plans(unet, tcfg, hw, n):
    """the plans of the last forward, read back: dict prefix -> a plan per sample (blocks that merged nothing are left out)"""
    forced = {}
    pre = RU.merged_prefixes(tcfg, unet.cfg["layers_per_block"])
    assert [RU.block_prefixes()[b] for b in unet.token_merging_blocks()] == pre
    for k, p in enumerate(pre):
        lv = RU.level_of(p)
        h, w = hw
        for _ in range(lv):
            h, w = (h + 1) // 2, (w + 1) // 2
        flat = unet.token_merging_plan(k)
        sp, dp = R.tables(h, w, 2, 2, tcfg["use_rand"], tcfg["seed"])
        r = R.merge_count(h * w, len(sp), tcfg["ratio"]) if dp else 0
        if r == 0:
            assert flat is None
            continue
        rows = flat.view(n, h * w)
        forced[p] = [R.plan_from_out_row(rows[s], sp, dp) for s in range(n)]
        assert all(q["r"] == r for q in forced[p])
    return forced


def test_off_is_the_plain_forward_bitwise(tiny, lib):
    """ratio = 0 and remove_token_merging(): the plain forward's bits and an identical implicit-GEMM launch log; ratio = 0.5 changes the output"""
    from tests import tuned_cases
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = _fwd_inputs(tiny, (8, 6))

    def logged():
        lib.ladi_igemm_launch_log(1)
        try:
            out = unet(xd, T0, encoder_hidden_states=ed).sample.float().cpu()
            torch.cuda.synchronize()
        finally:
            lib.ladi_igemm_launch_log(0)
        return out, tuned_cases.read_log(lib)
    unet(xd, T0, encoder_hidden_states=ed)          # the context upload and the first-use tile selection stay out of the logs
    plain, log_plain = logged()
    assert unet.token_merging is None and unet.token_merging_blocks() == []
    unet.set_token_merging(0.0)
    zero, log_zero = logged()
    assert unet.token_merging is None
    unet.set_token_merging(0.5)
    assert unet.token_merging == dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False,
                                      merge_mlp=False)
    on, log_on = logged()
    unet.remove_token_merging()
    off, log_off = logged()
    assert torch.equal(zero, plain) and torch.equal(off, plain)
    assert log_zero == log_plain and log_off == log_plain and log_on != log_plain
    assert torch.isfinite(on).all() and U.psnr(on, plain) < PSNR_DB
    with pytest.raises(ValueError):
        unet.set_token_merging(1.0)
    assert lib.ladi_unet_set_token_merging(unet.h, ctypes.byref(_lib.ToMeConfig(ratio=0.5, max_downsample=3, sx=2, sy=2, merge_attn=1))) == -1
    assert "max_downsample" in _lib.last_error() and unet.token_merging is None


FWD_CASES = {
    "attn": dict(ratio=0.5),
    "all": dict(ratio=0.5, merge_crossattn=True, merge_mlp=True),
    "attn_md2": dict(ratio=0.5, max_downsample=2),
    "all_md2_rand": dict(ratio=0.6, max_downsample=2, use_rand=True, seed=9, merge_crossattn=True, merge_mlp=True),
    "mlp_only_rand": dict(ratio=0.3, use_rand=True, seed=2, merge_attn=False, merge_mlp=True),
}


@pytest.mark.parametrize("hw", [(8, 6), (5, 3)])
@pytest.mark.parametrize("case", list(FWD_CASES) + ["attn+ip", "all+ip"])
def test_forward_with_forced_plans(tiny, case, hw):
    """NativeUNet tiny, B = 2, t = 481: every merged block's plan is read back and forced into ref_unet's forward; thresholds of
    tests/test_gpu_pag.py's forward comparison (rel-L2 <= 5e-3, PSNR >= 55 dB).  +ip: with an IP-Adapter image context set (one block at
    scale 0), the image term from the merged rows where the cross-attention merges; "plain" is then the unmerged forward with that context"""
    from ladi_vton_amd import tome
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = _fwd_inputs(tiny, hw)
    kw, ip = {}, None
    if case.endswith("+ip"):
        sd_ip, emb, tok = _adapter(tiny)
        kw, ip = dict(ip_image_embeds=emb.to(U.dev())), (sd_ip, tok, IP_SCALES)
    tcfg = tome.config(**FWD_CASES[case.split("+")[0]])
    plain = unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu()
    unet.set_token_merging(**FWD_CASES[case.split("+")[0]])
    got = unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu()
    forced = _device_plans(unet, tcfg, hw, 2)
    assert forced, "nothing merged"
    ref = RU.unet_forward(tiny["sd"]["unet"], tiny["ucfg"], x, T0, ehs, tome=(tcfg, forced, None, "proj_in"), ip=ip)
    ps, rl = U.psnr(got, ref), U.rel_l2(got, ref)
    print("ToMe forward %s %dx%d: PSNR %.2f dB, rel-L2 %.3g; against plain %.2f dB" % ((case,) + hw + (ps, rl, U.psnr(got, plain))))
    U.record_parity("tome_forward_tiny_%s_%dx%d" % ((case,) + hw), dict(psnr_db=round(ps, 2), rel_l2=rl))
    assert torch.isfinite(got).all() and rl <= REL_L2 and ps >= PSNR_DB, (ps, rl)
    assert not torch.equal(got, plain)
    assert torch.equal(unet(xd, T0, encoder_hidden_states=ed, **kw).sample.float().cpu(), got)     # and it is reproducible


def wiring_shares(sd, ucfg, x, ehs, tcfg):
    """CPU side of the wiring test -> (reference plans of the first merged block, d0, share with the metric after norm1, share with the
    metric before proj_in)"""
    first = RU.merged_prefixes(tcfg)[0]
    rec = {}

    def grab(metric):
        out = {}
        RU.unet_forward(sd, ucfg, x, T0, ehs, tome=(tcfg, None, lambda p, t, plans: out.setdefault(p, (t, plans)), metric))
        return out[first]
    t0, ref = grab("proj_in")
    h, w = x.shape[2:]
    sp, dp = R.tables(h, w, 2, 2, tcfg["use_rand"], tcfg["seed"])
    r = ref[0]["r"]
    n = x.shape[0]
    share = lambda plans: sum(R.plan_diff(plans[s], ref[s]) for s in range(n)) / n
    d0 = share([R.plan_of_metric(t0[s].half().float(), sp, dp, r, torch.float32) for s in range(n)])
    rec = (ref, d0, share(grab("norm1")[1]), share(grab("input")[1]), len(sp))
    return rec


def test_plan_wiring(tiny):
    """The first merged block's device plan against tome_ref's own plan from its fp32 block input, as the share of src tokens whose
    (merged?, partner) differ.  Bound: max(4 d0, 2 / Ns), d0 the share between plan(X_ref) and plan(fp16(X_ref)) on the CPU (the device input
    carries one convolution and one ResNet of fp16 error on top of that rounding).  With this seed (8 x 6 latents, Ns = 36, B = 2):
    d0 = 0.0000, bound = 2 / 36 = 0.0556, metric after norm1 0.1111, metric before proj_in 0.5833 (both mis-wirings lie above the bound);
    measured device share 0.0000 (BASELINE.md "Token merging")."""
    from ladi_vton_amd import tome
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = _fwd_inputs(tiny, (8, 6))
    tcfg = tome.config(0.5)
    ref, d0, d_norm1, d_input, Ns = wiring_shares(tiny["sd"]["unet"], tiny["ucfg"], x, ehs, tcfg)
    bound = max(4 * d0, 2.0 / Ns)
    unet.set_token_merging(0.5)
    unet(xd, T0, encoder_hidden_states=ed)
    dev = _device_plans(unet, tcfg, (8, 6), 2)[RU.merged_prefixes(tcfg)[0]]
    d_dev = sum(R.plan_diff(dev[s], ref[s]) for s in range(2)) / 2
    print("ToMe plan wiring: device share %.4f, bound %.4f (d0 %.4f), after norm1 %.4f, before proj_in %.4f" % (d_dev, bound, d0, d_norm1, d_input))
    U.record_parity("tome_plan_wiring", dict(device=d_dev, d0=d0, bound=bound, norm1=d_norm1, before_proj_in=d_input))
    assert bound < d_norm1 and bound < d_input
    assert d_dev <= bound, (d_dev, bound)


# ------------------------------------------------------------------------------------------------------------------ tiny model, end to end
STEPS = 4
TOME = dict(ratio=0.5, merge_crossattn=True, merge_mlp=True)


def _inputs(tiny, size=(64, 48)):
    key = ("inp",) + size
    if key not in tiny:
        inp = P.synthetic_inputs(2, size[0], size[1], L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny[key] = inp
    return tiny[key]


def _pipe(tiny, scheduler=None):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=scheduler or L.DDIMScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, fused=True, graph=True, steps=STEPS, **kw):
    inp, d = _inputs(tiny), U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=64, width=48, num_inference_steps=steps,
               output_type="np", fused=fused, use_graph=graph, noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _cached_run(tiny, key, tcfg, **kw):
    """one run per key on a fresh pipeline; the configuration lives in the UNet every pipeline of this module shares, so the caller's is put back"""
    if key not in tiny["run"]:
        unet = tiny["mod"]["unet"]
        saved = unet.token_merging
        unet.set_token_merging(**tcfg) if tcfg else unet.remove_token_merging()
        tiny["run"][key] = _call(tiny, _pipe(tiny), **kw)
        unet.set_token_merging(**saved) if saved else unet.remove_token_merging()
    return tiny["run"][key]


def _plain(tiny):
    return _cached_run(tiny, "plain", None)


def _merged(tiny, arm):
    return _cached_run(tiny, arm, TOME, fused=arm != "modular", graph=arm == "graph")


@pytest.mark.parametrize("arm", ["graph", "eager", "modular", "lanes"])
def test_loop_vs_reference(tiny, arm):
    """4 DDIM steps, all three sub-layers merged: a step callback reads the plans of every evaluation back, ref_tryon.tryon_reference runs
    with them forced; thresholds of tests/test_gpu_pag.py's end-to-end test (latents >= 40 dB, image >= 35 dB).  The callback changes
    nothing: the run equals the run without one bit for bit.  lanes: the graph run on two sample-group lanes (a merge that flips between one
    lane and two moves the result by more than rounding, so the lanes are held to the reference with their own plans, not to the one-lane run)"""
    from ladi_vton_amd import tome
    tcfg = tome.config(**TOME)
    unet = tiny["mod"]["unet"]
    pipe = _pipe(tiny)
    plain_lat = _plain(tiny)[1]
    pipe.apply_token_merging(**TOME)
    assert pipe.token_merging == tcfg
    if arm == "lanes":
        pipe.lanes = 2
    per_eval = []
    img, lat = _call(tiny, pipe, fused=arm != "modular", graph=arm != "eager",
                     callback=lambda i, t, latents: per_eval.append(_device_plans(unet, tcfg, (8, 6), 4)))
    assert len(per_eval) == STEPS
    ref_img, ref_lat = RT.tryon_reference(tiny["sd"]["unet"], tiny["ucfg"], tiny["sd"]["vae"], tiny["vcfg"], tiny["sd"]["emasc"], _inputs(tiny), STEPS,
                                          "ddim", tome=(tcfg, per_eval))
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    p_plain = U.psnr(lat, plain_lat)
    print("tiny ToMe %s: image %.2f dB, latents %.2f dB; against the plain run %.2f dB" % (arm, p_img, p_lat, p_plain))
    U.record_parity("tome_tiny_ddim_%s" % arm, dict(image_db=round(p_img, 2), latents_db=round(p_lat, 2)))
    assert torch.isfinite(lat).all() and p_lat >= LAT_DB and p_img >= IMG_DB, (p_img, p_lat)
    assert p_plain < LAT_DB, p_plain                                   # and it is not the plain loop
    if arm == "lanes":
        assert pipe.lib_lanes() == 2
    else:
        img_n, lat_n = _merged(tiny, arm)
        assert torch.equal(lat, lat_n) and torch.equal(img, img_n)


def test_graph_equals_eager_and_runs_repeat_bitwise(tiny):
    img_g, lat_g = _merged(tiny, "graph")
    img_e, lat_e = _merged(tiny, "eager")
    assert torch.equal(lat_g, lat_e) and torch.equal(img_g, img_e)
    pipe = _pipe(tiny)
    pipe.apply_token_merging(**TOME)
    a = _call(tiny, pipe)
    b = _call(tiny, pipe)                                              # the second call replays the captured graphs
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and torch.equal(a[1], lat_g)


@pytest.mark.parametrize("what", ["feature_cache", "pag_mid", "lcm2", "ip"])
def test_loop_with_other_switches(tiny, what):
    """token merging together with feature_cache = 2, PAG on the mid block, a 2-step LCM run and an IP-Adapter image prompt (one block at
    scale 0): the graph run is finite, equals the eager run bit for bit and differs from the same run without merging"""
    import ladi_vton_amd as L
    kw, steps, sched = {}, STEPS, None
    if what == "feature_cache":
        kw = dict(feature_cache=2)
    elif what == "pag_mid":
        kw = dict(pag_scale=3.0)
    elif what == "lcm2":
        steps, sched = 2, L.LCMScheduler()
    elif what == "ip":
        kw = dict(ip_adapter_image_embeds=_adapter(tiny)[1].to(U.dev()))
    pipe = _pipe(tiny, sched)

    def call(**k):                                                      # LCM draws step noise: every call gets its own seeded generator
        if what == "lcm2":
            k["generator"] = torch.Generator().manual_seed(31)
        return _call(tiny, pipe, **k)
    off = call(steps=steps, **kw)
    pipe.apply_token_merging(**TOME)
    on = call(steps=steps, **kw)
    eager = call(graph=False, steps=steps, **kw)
    assert torch.equal(on[1], eager[1]) and torch.equal(on[0], eager[0])
    assert torch.isfinite(on[1]).all() and not torch.equal(on[1], off[1])


def test_no_stale_graph(tiny):
    """one pipeline with use_graph: plain -> ratio 0.5 -> ratio 0.25 -> removed.  Every change alters the result, each merged run equals
    the run of a fresh pipeline at that configuration, and the last run is the plain run bit for bit"""
    pipe = _pipe(tiny)
    img_1, lat_1 = _call(tiny, pipe)
    pipe.apply_token_merging(**TOME)
    img_2, lat_2 = _call(tiny, pipe)
    pipe.apply_token_merging(**dict(TOME, ratio=0.25))
    img_3, lat_3 = _call(tiny, pipe)
    pipe.remove_token_merging()
    img_4, lat_4 = _call(tiny, pipe)
    assert torch.equal(lat_4, lat_1) and torch.equal(img_4, img_1) and torch.equal(lat_1, _plain(tiny)[1])
    assert torch.equal(lat_2, _merged(tiny, "graph")[1])
    fresh = _pipe(tiny)
    fresh.apply_token_merging(**dict(TOME, ratio=0.25))
    assert torch.equal(lat_3, _call(tiny, fresh)[1])
    for a, b, what in ((lat_1, lat_2, "plain / 0.5"), (lat_2, lat_3, "0.5 / 0.25"), (lat_1, lat_3, "plain / 0.25")):
        print("ToMe runs %s: latents %.2f dB apart" % (what, U.psnr(a, b)))
        assert not torch.equal(a, b)


def test_misuse(tiny):
    pipe = _pipe(tiny)
    for bad in (dict(ratio=1.0), dict(ratio=-0.1), dict(ratio=float("nan")), dict(sx=4), dict(sy=3), dict(max_downsample=0), dict(max_downsample=4),
                dict(merge_attn=False)):
        with pytest.raises(ValueError):
            pipe.apply_token_merging(**bad)
    assert pipe.token_merging is None
    pipe.apply_token_merging(0.5)
    pipe.set_pag_applied_layers(["down.block_0", "mid"])
    with pytest.raises(ValueError, match="merge tokens"):
        _call(tiny, pipe, pag_scale=3.0)
    pipe.set_pag_applied_layers("mid")
    pipe.remove_token_merging()
    assert torch.equal(_call(tiny, pipe)[1], _plain(tiny)[1])           # the handle is as it was
    other = _pipe(tiny)
    other.unet = SimpleNamespace(config=tiny["mod"]["unet"].config)
    with pytest.raises(ValueError, match="native UNet"):
        other.apply_token_merging(0.5)
    with pytest.raises(ValueError, match="native UNet"):
        other.remove_token_merging()
    # the forward itself refuses perturbed samples in a block that merges
    unet = tiny["mod"]["unet"]
    x, ehs, xd, ed = _fwd_inputs(tiny, (8, 6))
    unet.set_token_merging(0.5)
    unet.set_pag_applied_layers("down.block_0")
    with pytest.raises(_lib.NativeError, match="merges tokens"):
        unet(torch.cat([xd, xd]), T0, encoder_hidden_states=torch.cat([ed, ed]), pag_first=2)
