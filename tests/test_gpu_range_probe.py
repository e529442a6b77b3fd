"""fp16 range probe (csrc/probe.hip, ladi_probe_*, ladi_vton_amd.RangeProbe) through the C ABI: the kernel is exact on every view shape, slots
accumulate and reset, every module reports the documented points without changing a bit of its output, inner points agree with the fp32
oracle, and a checkpoint made to overflow in one known layer is reported at exactly that layer -- stand-alone and inside the fused loop."""
import pytest
import torch

from oracle import configs as C
from oracle import pipeline as P
from tests import range_probe_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
# worst |native - oracle| / oracle over the UNet's probe points, measured on MI355X by tools/range_probe_parity.py
# (profiles/range_probe_parity.json): tiny configuration 1.209e-3 (up_blocks.0.resnets.0), released configuration 8.76e-4
# (up_blocks.2.attentions.2, one 64 x 48 forward).  The test asserts 4x the tiny figure
# (margin for box-to-box and tile-selection differences in accumulation order); a probe that is off by one layer differs by tens of percent.
MEASURED_TINY_WORST_REL = 1.209e-3
INNER_POINT_BOUND = 4 * MEASURED_TINY_WORST_REL
assert INNER_POINT_BOUND < 0.05


def _op_absmax(view_ptr, rows, Cc, ld, am, nf):
    from ladi_vton_amd import _lib
    lib = _lib.load()
    rc = lib.ladi_op_absmax(view_ptr, rows, Cc, ld, _lib.ptr(am), _lib.ptr(nf), _lib.stream_ptr())
    assert rc == 0, _lib.last_error()


def _poisoned(rows, Cc, ld, off, valid):
    """fp16 buffer holding a [rows][ld] view that starts `off` elements (+ 2 poisoned rows) in; the view's first Cc lanes = valid [rows][Cc],
    everything else (padding lanes, rows before and after, the slack) cycles through inf, nan, 65504 -> (buffer, element offset of the view)"""
    pre = post = 2
    total = off + (pre + rows + post) * ld + 8
    buf = torch.tensor([INF, NAN, 65504.0], dtype=torch.float16).repeat(total // 3 + 1)[:total].clone()
    start = off + pre * ld
    v = buf[start:start + rows * ld].view(rows, ld)
    v[:, :Cc] = valid
    return buf, start


def _expected(valid):
    x = valid.float()
    fin = torch.isfinite(x)
    return (float(x[fin].abs().max()) if bool(fin.any()) else 0.0), int((~fin).sum())


def _specials(valid, vals):
    flat = valid.view(-1)
    step = max(1, flat.numel() // (len(vals) + 1))
    for i, s in enumerate(vals):
        flat[min(i * step + step // 2, flat.numel() - 1) if flat.numel() > len(vals) else i % flat.numel()] = s


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows,Cc,ld", [(1, 1, 1), (7, 31, 64), (5, 4, 4), (3, 8, 8), (3072, 320, 320), (33, 1280, 1288)])
def test_kernel_is_exact_on_padded_offset_views(rows, Cc, ld, off):
    """expected = x[isfinite].abs().max() and (~isfinite).sum() from torch, compared with ==; padding lanes and the rows around the view hold
    inf / nan / 65504 and must not show"""
    g = torch.Generator().manual_seed(rows * 7 + Cc)
    base = (torch.randn((rows, Cc), generator=g) * 50).half()
    cases = {}
    a = base.clone(); _specials(a, [INF, -INF, NAN, -65504.0, -0.0, 6e-8, -1.2e-7]); cases["with -65504"] = a
    b = base.clone().clamp(-200, 200); _specials(b, [-0.0, 6e-8, INF, NAN, -INF, -1.2e-7]); cases["small finite values"] = b
    cases["all non-finite"] = torch.tensor([INF, NAN, -INF], dtype=torch.float16).repeat(rows * Cc // 3 + 1)[:rows * Cc].view(rows, Cc).clone()
    cases["subnormals and zeros only"] = torch.tensor([6e-8, -0.0, -1.8e-7, 0.0], dtype=torch.float16).repeat(rows * Cc // 4 + 1)[:rows * Cc].view(rows, Cc).clone()
    for what, valid in cases.items():
        buf, start = _poisoned(rows, Cc, ld, off, valid)
        dbuf = buf.to(U.dev())
        am = torch.zeros(1, dtype=torch.float32, device=U.dev())
        nf = torch.zeros(1, dtype=torch.int32, device=U.dev())
        _op_absmax(dbuf.data_ptr() + 2 * start, rows, Cc, ld, am, nf)
        torch.cuda.synchronize()
        exp_m, exp_c = _expected(valid)
        assert (float(am), int(nf)) == (exp_m, exp_c), (what, float(am), int(nf), exp_m, exp_c)
    assert _expected(cases["all non-finite"]) == (0.0, rows * Cc)


def test_op_rejects_bad_arguments_and_accumulates():
    """two launches into the same words: the max of both and the sum of the counts"""
    from ladi_vton_amd import _lib
    lib = _lib.load()
    x1 = torch.tensor([[1.0, -3.0, INF, 2.0]], dtype=torch.float16, device=U.dev())
    x2 = torch.tensor([[NAN, 7.5, NAN, -0.5]], dtype=torch.float16, device=U.dev())
    am = torch.zeros(1, dtype=torch.float32, device=U.dev())
    nf = torch.zeros(1, dtype=torch.int32, device=U.dev())
    _op_absmax(x2.data_ptr(), 1, 4, 4, am, nf)
    _op_absmax(x1.data_ptr(), 1, 4, 4, am, nf)
    torch.cuda.synchronize()
    assert (float(am), int(nf)) == (7.5, 3)
    assert lib.ladi_op_absmax(_lib.ptr(x1), 1, 4, 3, _lib.ptr(am), _lib.ptr(nf), _lib.stream_ptr()) != 0      # ld < C
    assert lib.ladi_op_absmax(_lib.ptr(x1), 1, 0, 4, _lib.ptr(am), _lib.ptr(nf), _lib.stream_ptr()) != 0      # C < 1


# --------------------------------------------------------------------------------------------------------------- modules
@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 31, 16, 16), generator=g).half().float()
    ehs = torch.randn((2, 8, ucfg["cross_attention_dim"]), generator=g).half().float()
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, x=x, ehs=ehs, t=481)


@pytest.fixture(scope="module")
def unet_ref(tiny):
    """fp32 oracle magnitudes of every UNet probe point for the shared input (computed once)"""
    return R.unet_point_absmax(tiny["sd"]["unet"], tiny["ucfg"], tiny["x"], tiny["t"], tiny["ehs"])[0]


def _unet_names_tiny():
    """the documented enumeration, written out for layers_per_block = 2"""
    n = ["conv_in"]
    for i in range(4):
        for j in range(2):
            n += ["down_blocks.%d.resnets.%d" % (i, j)] + (["down_blocks.%d.attentions.%d" % (i, j)] if i < 3 else [])
        n += ["down_blocks.%d.downsamplers.0" % i] if i < 3 else []
    n += ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
    for i in range(4):
        for j in range(3):
            n += ["up_blocks.%d.resnets.%d" % (i, j)] + (["up_blocks.%d.attentions.%d" % (i, j)] if i > 0 else [])
        n += ["up_blocks.%d.upsamplers.0" % i] if i < 3 else []
    return n + ["conv_out"]


def _unet(unet, tiny, x=None):
    out = unet((tiny["x"] if x is None else x).to(U.dev()), tiny["t"], encoder_hidden_states=tiny["ehs"].to(U.dev())).sample
    torch.cuda.synchronize()
    return out


def _probed_unet_run(unet, tiny):
    """-> (report of one forward of `unet` under a fresh probe, the output)"""
    import ladi_vton_amd as L
    probe = L.RangeProbe().attach(unet)
    try:
        out = _unet(unet, tiny)
        return probe.report(), out
    finally:
        probe.detach()


def test_unet_points_names_output_bits_and_reset(tiny):
    import ladi_vton_amd as L
    from ladi_vton_amd.probe import unet_point_names
    unet = tiny["mod"]["unet"]
    plain = _unet(unet, tiny)
    probe = L.RangeProbe().attach(unet)
    try:
        out = _unet(unet, tiny)
        rep = probe.report()
        assert [r[0] for r in rep] == _unet_names_tiny() == unet_point_names(tiny["ucfg"])
        assert torch.equal(out, plain)                                      # attaching a probe changes no bit of the output
        d = {r[0]: r for r in rep}
        assert d["conv_out"][1] == float(out.abs().max()) and all(r[3] == 0 for r in rep)
        assert d["conv_out"][2] == d["conv_out"][1] / 65504.0 and probe.first_nonfinite() is None
        # accumulation: a second forward on a 4x larger input leaves the max of both; reset() zeroes everything
        out4 = _unet(unet, tiny, tiny["x"] * 4)
        rep2 = {r[0]: r for r in probe.report()}
        assert rep2["conv_out"][1] == max(float(out.abs().max()), float(out4.abs().max()))
        assert all(rep2[k][1] >= d[k][1] for k in d) and rep2["conv_in"][1] > d["conv_in"][1]
        probe.reset()
        assert all(r[1] == 0.0 and r[3] == 0 for r in probe.report())
        assert [r[0] for r in probe.report()] == unet_point_names(tiny["ucfg"])
    finally:
        probe.detach()
    assert torch.equal(_unet(unet, tiny), plain)                            # and detaching restores the plain path


def test_vae_encode_and_emasc_points_match_the_returned_tensors(tiny):
    import ladi_vton_amd as L
    from ladi_vton_amd.probe import emasc_point_names, vae_encoder_point_names
    vae, emasc = tiny["mod"]["vae"], tiny["mod"]["emasc"]
    x = P.synthetic_inputs(2, 64, 64, L=4, D=8)["image"].to(U.dev())
    enc0, feats0 = vae.encode(x)
    outs0 = emasc([f.clone() for f in feats0[1:]])
    torch.cuda.synchronize()
    probe = L.RangeProbe().attach(vae, emasc)
    try:
        enc, feats = vae.encode(x)
        outs = emasc([f.clone() for f in feats[1:]])
        torch.cuda.synchronize()
        rep = probe.report()
        assert [r[0] for r in rep] == vae_encoder_point_names() + emasc_point_names(tiny["ecfg"])
        d = {r[0]: r[1] for r in rep}
        assert all(r[3] == 0 for r in rep)
        assert torch.equal(enc.latent_dist.parameters, enc0.latent_dist.parameters)
        assert d["quant_conv"] == float(enc.latent_dist.parameters.abs().max())
        # feats = [x, conv_in out, = , in(down 1) = out(down 0), in(down 2), in(down 3)]
        for name, i in (("encoder.conv_in", 1), ("encoder.down_blocks.0", 3), ("encoder.down_blocks.1", 4), ("encoder.down_blocks.2", 5)):
            assert torch.equal(feats[i], feats0[i])
            assert d[name] == float(feats[i].float().abs().max()), name
        for i in range(5):
            assert torch.equal(outs[i], outs0[i])
            assert d["emasc.%d" % i] == float(outs[i].float().abs().max()), i
    finally:
        probe.detach()


def test_inner_points_agree_with_the_fp32_oracle(tiny, unet_ref):
    rep, _ = _probed_unet_run(tiny["mod"]["unet"], tiny)
    rel = {name: abs(a - unet_ref[name]) / unet_ref[name] for name, a, _, _ in rep}
    worst = max(rel, key=rel.get)
    print("range probe vs oracle: worst relative difference %.3e at %s" % (rel[worst], worst))
    assert list(rel) == list(unet_ref)
    assert rel[worst] <= INNER_POINT_BOUND, (worst, rel[worst])


@pytest.mark.parametrize("weights,point", [("down_blocks.1.resnets.0.conv2", "down_blocks.1.resnets.0"),
                                           ("down_blocks.1.attentions.0.proj_out", "down_blocks.1.attentions.0")])
def test_stress_overflow_is_reported_at_the_layer_that_overflowed(tiny, weights, point):
    """the scaled-activation stress test: one layer's output weights x 2^k, k chosen on the CPU so that the fp32 oracle exceeds 4 x 65504 at
    that point.  The probe names exactly that layer first, everything before it is bit-identical to the unscaled run, and the NaNs reach conv_out"""
    import ladi_vton_amd as L
    sd, cfg = tiny["sd"]["unet"], tiny["ucfg"]
    k, ref_max = R.overflow_exponent(sd, cfg, tiny["x"], tiny["t"], tiny["ehs"], weights, point)
    assert ref_max > 4 * 65504.0
    base, _ = _probed_unet_run(tiny["mod"]["unet"], tiny)
    stressed = L.NativeUNet(cfg, R.scaled_checkpoint(sd, weights, 2.0 ** k))
    probe = L.RangeProbe().attach(stressed)
    try:
        _unet(stressed, tiny)
        rep = probe.report()
        assert probe.first_nonfinite() == point, (k, probe.first_nonfinite())
    finally:
        probe.detach()
    names = [r[0] for r in rep]
    at = names.index(point)
    assert rep[:at] == base[:at] and all(r[3] == 0 for r in rep[:at])
    assert rep[at][3] > 0 and rep[-1][0] == "conv_out" and rep[-1][3] > 0


# --------------------------------------------------------------------------------------------------------------- fused loop
def _pipe(tiny, unet=None):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=unet or tiny["mod"]["unet"],
                                           scheduler=L.DDIMScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(pipe, tiny, graph, guidance=7.5, **kw):
    B, H, W = 1, 128, 128
    inp = P.synthetic_inputs(B, H, W, L=8, D=tiny["ucfg"]["cross_attention_dim"])
    d = U.dev()
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].half().to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].half().to(d), height=H, width=W, num_inference_steps=3,
               guidance_scale=guidance, output_type="np", use_graph=graph,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images)


@pytest.mark.parametrize("graph", [True, False])
def test_fused_loop_with_probe(tiny, graph):
    import ladi_vton_amd as L
    from ladi_vton_amd.probe import emasc_point_names, unet_point_names, vae_decoder_point_names, vae_encoder_point_names
    pipe = _pipe(tiny)
    off = _call(pipe, tiny, graph)
    probe = L.RangeProbe()
    pipe.range_probe = probe
    try:
        on = _call(pipe, tiny, graph)
        rep1 = probe.report()
        assert torch.equal(on, off)                                         # images bit-equal with the probe on and off
        assert [r[0] for r in rep1] == (vae_encoder_point_names() + emasc_point_names(tiny["ecfg"]) + unet_point_names(tiny["ucfg"]) +
                                        vae_decoder_point_names())
        assert all(r[3] == 0 for r in rep1) and all(r[1] > 0 for r in rep1)
        # a second run (the slots are zeroed at its start) reproduces the first; so does one after an explicit reset()
        assert torch.equal(_call(pipe, tiny, graph), off) and probe.report() == rep1
        probe.reset()
        assert torch.equal(_call(pipe, tiny, graph), off) and probe.report() == rep1
        # probe, no probe, probe again: a graph captured without the probe launches is not replayed with it, nor the other way round
        pipe.range_probe = None
        assert torch.equal(_call(pipe, tiny, graph), off)
        probe.reset()
        assert all(r[1] == 0.0 and r[3] == 0 for r in probe.report())       # the run without the probe wrote nothing into it
        pipe.range_probe = probe
        assert torch.equal(_call(pipe, tiny, graph), off) and probe.report() == rep1
        # accumulation over every evaluation (eager first one + replays): without classifier-free guidance the traced noise prediction IS
        # the UNet output of each evaluation (with it the trace holds the guided combination), so its maximum over the run is the slot
        pipe.trace_evals = 3
        _call(pipe, tiny, graph, guidance=1.0)
        d = {r[0]: r for r in probe.report()}
        tr = pipe.last_trace["noise_pred"]
        per_eval = [float(tr[i].abs().max()) for i in range(3)]
        print("conv_out slot %r, per-evaluation maxima %r" % (d["conv_out"][1], per_eval))
        assert tr.shape[0] == 3 and d["conv_out"][1] == max(per_eval)
        # the later evaluations on their own (with use_graph the replays of the captured graph): a step callback zeroes the slots after
        # evaluation 0, the eager one, so what the slot holds at the end was written by evaluations 1 and 2 alone, wherever the run's
        # maximum lies.  This leans on how the loop runs a callback today (runtime_tryon.cpp callback_point): on the host BETWEEN two
        # evaluations, after the loop's stream was synchronised, and the loop's next launch waits for what the callback queued on the
        # caller's stream -- so the reset is ordered after evaluation 0's probe launches and before evaluation 1's.  A loop that let
        # evaluations run ahead of the callback would make this reset race with the slots: then this check has to go another way.

        def zero_after_first(i, t, latents):
            if i == 0:
                probe.reset()

        _call(pipe, tiny, graph, guidance=1.0, callback=zero_after_first)
        d = {r[0]: r for r in probe.report()}
        tr = pipe.last_trace["noise_pred"]
        per_eval = [float(tr[i].abs().max()) for i in range(3)]
        print("conv_out slot after a reset behind evaluation 0 %r, per-evaluation maxima %r" % (d["conv_out"][1], per_eval))
        assert tr.shape[0] == 3 and d["conv_out"][1] == max(per_eval[1:]) and d["conv_in"][1] > 0 and d["conv_in"][3] == 0
    finally:
        pipe.range_probe = None
        pipe.trace_evals = 0


def test_fused_loop_raises_at_the_stressed_layer(tiny):
    import ladi_vton_amd as L
    sd, cfg = tiny["sd"]["unet"], tiny["ucfg"]
    weights, point = "down_blocks.1.resnets.0.conv2", "down_blocks.1.resnets.0"
    k, _ = R.overflow_exponent(sd, cfg, tiny["x"], tiny["t"], tiny["ehs"], weights, point)
    # the loop's inputs are not the ones k was chosen for: 2^4 more; its own VAE, whose automatic range shift the NaN latents raise
    pipe = _pipe(tiny, unet=L.NativeUNet(cfg, R.scaled_checkpoint(sd, weights, 2.0 ** (k + 4))))
    probe = L.RangeProbe()
    probe.raise_on_nonfinite = True
    pipe.range_probe = probe
    shared_vae = pipe.vae
    pipe.vae = L.NativeVAE(tiny["vcfg"], tiny["sd"]["vae"])                 # replaced after the probe was set: the call attaches to this one
    try:
        with pytest.raises(L.NativeError, match="fp16 range exceeded first at " + point.replace(".", r"\.")):
            _call(pipe, tiny, True)
        rep_ = probe.report()
        assert probe.first_nonfinite() == point and rep_[[r[0] for r in rep_].index("conv_out")][3] > 0
        # the probe followed the pipeline to its new VAE and left the one it was first attached to
        enc = dict((r[0], r) for r in rep_)["encoder.conv_in"]
        assert enc[1] > 0 and all(m is not shared_vae for m in probe._attached) and any(m is pipe.vae for m in probe._attached)
        probe.reset()
        shared_vae.encode(P.synthetic_inputs(1, 64, 64, L=4, D=8)["image"].to(U.dev()))
        torch.cuda.synchronize()
        assert all(r[1] == 0.0 and r[3] == 0 for r in probe.report())
    finally:
        pipe.range_probe = None


def test_decoder_points_are_reported_at_true_scale(tiny):
    """vae.range_shift = 4 stores the decoder's stream x 2^-4; the probe reports stored / 2^-4: equal to the shift-0 report within the fp16
    rounding of the stored stream (relative 2^-10)"""
    import ladi_vton_amd as L
    from ladi_vton_amd.probe import vae_decoder_point_names
    vae = tiny["mod"]["vae"]
    z = torch.randn((1, 4, 16, 12), generator=torch.Generator().manual_seed(3)).to(U.dev())
    probe = L.RangeProbe().attach(vae)
    reps = {}
    try:
        for shift in (0, 4):
            vae.range_shift = shift
            probe.reset()
            vae.decode(z)
            torch.cuda.synchronize()
            assert vae.last_range_shift == shift
            reps[shift] = probe.report()
    finally:
        vae.range_shift = "auto"
        probe.detach()
    assert [r[0] for r in reps[0]] == vae_decoder_point_names()
    for r0, r4 in zip(reps[0], reps[4]):
        assert r0[3] == 0 and r4[3] == 0 and r0[1] > 0
        assert abs(r4[1] - r0[1]) <= r0[1] * 2.0 ** -10, (r0, r4)


def test_destroying_an_attached_probe_is_refused(tiny, lib):
    """a module that still points at a destroyed probe would launch into freed memory: ladi_probe_destroy keeps such a probe and says so;
    once detached (or once the module is gone) it destroys"""
    from ladi_vton_amd import _lib
    unet = tiny["mod"]["unet"]
    h = lib.ladi_probe_create(64)
    assert h
    try:
        assert lib.ladi_unet_attach_probe(unet.h, h) == 0
        lib.ladi_probe_destroy(h)
        assert "still attached to 1 module" in _lib.last_error()
        assert lib.ladi_probe_count(h) == 0 and lib.ladi_probe_reset(h, _lib.stream_ptr()) == 0      # alive and usable
        _unet(unet, tiny)
        assert lib.ladi_probe_count(h) == len(_unet_names_tiny())
    finally:
        assert lib.ladi_unet_attach_probe(unet.h, None) == 0
        lib.ladi_probe_destroy(h)
