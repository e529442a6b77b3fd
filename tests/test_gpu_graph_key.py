"""The fused loop's graph key (runtime.h GraphKey) end to end: ONE pipeline handle with use_graph runs the plain run A, another setting B and A
again, for every setting a captured launch depends on.  The third run is bit-equal to the first (A's graphs are not B's), B is bit-equal to B
on a fresh handle (B's graphs are not A's), and A and B differ, which is what makes a stale replay visible.  Tiny models at 64x48, DDIM with
5 steps: evaluation 0 runs eagerly and with 5 evaluations every form of a run replays from a graph at least once.  FreeU and PAG have their
own test_no_stale_graph (test_gpu_freeu.py, test_gpu_pag.py)."""
import pytest
import torch

from ladi_vton_amd import _lib
from ladi_vton_amd._lib import ptr
from oracle import configs as C
from oracle import pipeline as P
from tests import util as U

pytestmark = pytest.mark.gpu

STEPS = 5
PLAIN = dict()
# the keywords of the pipeline call; "size", "lanes" and "seed" (of the step-noise generator) are this module's own
SETTINGS = {
    "scalar5": dict(guidance_scale=5.0),
    "rescale05": dict(guidance_rescale=0.5),
    "rescale07": dict(guidance_rescale=0.7),
    "cutoff": dict(guidance_scale=[7.5, 7.5, 7.5, 1.0, 1.0]),
    "cache_b0": dict(feature_cache={"interval": 2, "branch": 0}),
    "cache_b1": dict(feature_cache={"interval": 2, "branch": 1}),
    "preserve": dict(preserve_unmasked="latents"),
    "eta": dict(eta=0.5, seed=5),
    "lanes2": dict(lanes=2),
    "size128": dict(size=(128, 96)),
}
# (A, B): A is the plain run at guidance 7.5, or the setting B is told apart from
PAIRS = [(None, "scalar5"), (None, "rescale05"), ("rescale05", "rescale07"), (None, "cutoff"), (None, "cache_b0"), ("cache_b0", "cache_b1"),
         (None, "preserve"), (None, "eta"), (None, "lanes2"), (None, "size128")]


@pytest.fixture(scope="module")
def tiny():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    mods = dict(unet=L.NativeUNet(ucfg, C.synth_state_dict(C.unet_shapes(ucfg), "unet.")),
                vae=L.NativeVAE(vcfg, C.synth_state_dict(C.vae_shapes(vcfg), "vae.")),
                emasc=L.NativeEMASC(ecfg, C.synth_state_dict(C.emasc_shapes(ecfg), "emasc.")))
    t = dict(ucfg=ucfg, mod=mods, inp={}, fresh={})
    t["pipe"] = _pipe(t)           # the one handle every test of this module runs on
    return t


def _pipe(tiny):
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=L.DDIMScheduler(), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def _call(tiny, pipe, name):
    """one fused use_graph run of a setting (None: the plain run) -> (images, latents)"""
    kw = dict(SETTINGS[name]) if name else dict(PLAIN)
    size, seed = kw.pop("size", (64, 48)), kw.pop("seed", None)
    pipe.lanes = kw.pop("lanes", 1)
    if size not in tiny["inp"]:
        inp = P.synthetic_inputs(2, size[0], size[1], L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny["inp"][size] = inp
    inp, d = tiny["inp"][size], U.dev()
    if seed is not None:
        kw["generator"] = torch.Generator().manual_seed(seed)
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=size[0], width=size[1], num_inference_steps=STEPS,
               output_type="np", fused=True, use_graph=True, noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def _fresh(tiny, name):
    """the setting's run on a handle that never ran anything else, once per module"""
    if name not in tiny["fresh"]:
        tiny["fresh"][name] = _call(tiny, _pipe(tiny), name)
    return tiny["fresh"][name]


def _same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


@pytest.mark.parametrize("a,b", PAIRS, ids=["%s-%s" % (a or "plain", b) for a, b in PAIRS])
def test_a_b_a_on_one_handle(tiny, a, b):
    pipe = tiny["pipe"]
    run_a = _call(tiny, pipe, a)
    run_b = _call(tiny, pipe, b)
    again = _call(tiny, pipe, a)
    assert _same(again, run_a)
    assert _same(run_a, _fresh(tiny, a))
    if b == "lanes2":
        # lanes change the per-launch batch, and with it the tile selection: the threshold of test_unet_lanes_match_single_lane (latents
        # >= 45 dB) against the single-lane run and against a fresh two-lane handle, in place of bit-equality
        assert pipe.lib_lanes() == 1        # `again` ran last
        for what, other in (("one lane", run_a), ("a fresh handle", _fresh(tiny, b))):
            p = U.psnr(run_b[1], other[1])
            print("two lanes against %s: latents %.2f dB" % (what, p))
            assert p >= 45.0, (what, p)
        return
    assert _same(run_b, _fresh(tiny, b))
    assert run_b[0].shape != run_a[0].shape or not torch.equal(run_b[1], run_a[1])


def test_cond_only_and_shallow_counts_follow_the_setting(tiny):
    """the forms the runs above replay: the cut-off's two cond-only evaluations, the cache's two shallow ones, none in the plain run"""
    pipe = tiny["pipe"]
    for name, cond, shallow in ((None, 0, 0), ("cutoff", 2, 0), ("cache_b0", 0, 2), (None, 0, 0)):
        _call(tiny, pipe, name)
        assert (pipe.cond_only_evals(), pipe.shallow_evals) == (cond, shallow), name


class _TraceInto:
    """the loaded library with ladi_tryon_set_trace pointed at buffers the test owns: the pipeline hands the loop a fresh trace tensor per
    call and frees it afterwards, so a write through a stale graph could not be seen there"""

    def __init__(self, lib, eps, lat):
        self._lib, self._eps, self._lat = lib, eps, lat

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ladi_tryon_set_trace(self, h, eps, lat, cap):
        if cap > 0:
            return self._lib.ladi_tryon_set_trace(h, ptr(self._eps), ptr(self._lat), cap)
        return self._lib.ladi_tryon_set_trace(h, None, None, 0)


def test_trace_buffer_is_written_when_set_and_left_alone_when_cleared(tiny, lib, monkeypatch):
    pipe = tiny["pipe"]
    plain = _call(tiny, pipe, None)
    eps = torch.zeros((STEPS, 2, 8 * 6, 4), dtype=torch.float32, device=U.dev())
    lat = torch.zeros_like(eps)
    monkeypatch.setattr(_lib, "_lib", _TraceInto(lib, eps, lat))
    try:
        pipe.trace_evals = STEPS
        assert _same(_call(tiny, pipe, None), plain)
        torch.cuda.synchronize()
        assert all(float(eps[i].abs().max()) > 0 and float(lat[i].abs().max()) > 0 for i in range(STEPS))
        pipe.trace_evals = 0
        eps.fill_(float("nan"))
        lat.fill_(float("nan"))
        assert _same(_call(tiny, pipe, None), plain)
        torch.cuda.synchronize()
        assert bool(torch.isnan(eps).all()) and bool(torch.isnan(lat).all())
    finally:
        pipe.trace_evals = 0


def test_probe_slots_are_written_when_attached_and_left_alone_when_detached(tiny):
    import ladi_vton_amd as L
    pipe = tiny["pipe"]
    plain = _call(tiny, pipe, None)
    probe = L.RangeProbe()
    pipe.range_probe = probe
    try:
        assert _same(_call(tiny, pipe, None), plain)
        rep = probe.report()
        assert rep and all(r[1] > 0 and r[3] == 0 for r in rep)
        pipe.range_probe = None
        probe.reset()
        assert _same(_call(tiny, pipe, None), plain)
        assert all(r[1] == 0.0 and r[3] == 0 for r in probe.report())
    finally:
        pipe.range_probe = None
