"""Keeping the unmasked region (`preserve_unmasked`) on the host, no GPU: the native blend coefficients (ladi_sched_keep_coeffs) against the
scheduler mirrors' add_noise in float64, the argument refusals of the pipeline and of the setter, and the sanity of tests/preserve_ref.py: with
nothing to keep its loop is the loop of tests/guidance_ref.py exactly, with everything to keep the final latents are z0."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import pipeline as P
from tests import guidance_ref as G
from tests import preserve_ref as R
from tests import strength_ref as SR

KIND = {"ddim": 0, "pndm": 1, "lms": 2, "dpmpp2m": 3, "euler": 4, "euler_a": 5}
NEW_SYMBOLS = ("ladi_tryon_set_preserve", "ladi_sched_keep_coeffs", "ladi_op_mask_pool8", "ladi_op_mask_feather", "ladi_op_image_composite",
               "ladi_op_sched_run_keep")


def lib_error():
    from ladi_vton_amd import _lib
    return _lib.last_error()


def _coeffs(lib, code, n, first_step, cap=None):
    ac = P.alphas_cumprod().contiguous()
    cap = n + 2 if cap is None else cap
    out = (ctypes.c_float * (2 * max(cap, 1)))()
    cnt = lib.ladi_sched_keep_coeffs(code, n, ctypes.c_void_p(ac.data_ptr()), first_step, out, cap)
    if cnt < 0:
        return cnt, lib_error()
    return np.array(list(out[:2 * cnt]), dtype=np.float32).reshape(cnt, 2)


def test_new_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------------------------ blend coefficients
@pytest.mark.parametrize("n", [2, 8, 50])
@pytest.mark.parametrize("kind", list(KIND))
def test_keep_coeffs_are_the_mirrors_add_noise_at_the_next_timestep(lib, kind, n):
    """whole runs and tails (first_step mid-run and the last admissible one): k_x, k_n of add_noise at timesteps[i + 1] in float64, relative
    error <= 1e-6 (an fp32 holding a float64 value: 2^-24 ~ 6e-8 with margin for the fp32 sigmas' own rounding); the last row is (1, 0)"""
    last = n - 2 if kind == "pndm" else n - 1
    for first_step in sorted({0, n // 2, last} & set(range(0, last + 1))):
        got = _coeffs(lib, KIND[kind], n, first_step)
        assert not isinstance(got, tuple), got
        s = SR.make_mirror(kind)
        s.set_timesteps(n, first_step=first_step) if first_step else s.set_timesteps(n)
        want = np.array(R.keep_coeffs(s), dtype=np.float64)
        assert got.shape == want.shape == (len(s.timesteps), 2), (got.shape, want.shape)
        assert tuple(got[-1]) == (1.0, 0.0)
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
        err[want == 0] = np.abs(got.astype(np.float64))[want == 0]
        assert err.max() <= 1e-6, (first_step, err.max())
        if kind in SR.SIGMA_KINDS:
            assert (got[:, 0] == 1.0).all()
        else:
            assert np.allclose(got[:, 0].astype(np.float64) ** 2 + got[:, 1].astype(np.float64) ** 2, 1.0, atol=1e-6)


def test_keep_coeffs_one_step_is_refused_like_the_table(lib):
    """the step table needs 2 steps (num_inference_steps out of range [2, 1000]); the coefficients follow it"""
    for kind in KIND.values():
        got = _coeffs(lib, kind, 1, 0)
        assert isinstance(got, tuple) and got[0] < 0 and "num_inference_steps" in got[1]


def test_keep_coeffs_refusals(lib):
    rc, msg = _coeffs(lib, 0, 8, 0, cap=4)
    assert rc < 0 and "too small" in msg
    rc, msg = _coeffs(lib, 0, 8, 8)
    assert rc < 0 and "first_step" in msg
    rc, msg = _coeffs(lib, 1, 8, 7)
    assert rc < 0 and "PNDM tail" in msg
    rc, msg = _coeffs(lib, 9, 8, 0)
    assert rc < 0 and "kind" in msg
    assert lib.ladi_sched_keep_coeffs(0, 8, None, 0, None, 10) < 0


def test_pndm_repeated_timestep_repeats_its_row(lib):
    """evaluations [u0, u1, u1, u2, ..]: after evaluation 0 and after evaluation 1 the latents belong to u1"""
    got = _coeffs(lib, KIND["pndm"], 8, 0)
    assert got.shape == (9, 2) and tuple(got[0]) == tuple(got[1]) and tuple(got[1]) != tuple(got[2])


# ------------------------------------------------------------------------------------------------------------------ setter
def test_setter_refuses_bad_arguments(lib):
    f = lib.ladi_tryon_set_preserve
    assert f(None, 4, 0.0) < 0 and "mode bits" in lib_error()
    assert f(None, -1, 0.0) < 0 and "mode bits" in lib_error()
    assert f(None, 2, -0.5) < 0 and "outside [0, 32]" in lib_error()
    assert f(None, 2, 32.5) < 0 and "outside [0, 32]" in lib_error()
    assert f(None, 3, float("nan")) < 0 and "outside [0, 32]" in lib_error()
    assert f(None, 1, 2.0) < 0 and "pixels" in lib_error()
    assert f(None, 0, 2.0) < 0 and "pixels" in lib_error()
    assert f(None, 0, 0.0) < 0 and "null handle" in lib_error()


# ------------------------------------------------------------------------------------------------------------------ pipeline arguments
class _Recorded(Exception):
    pass


def _cpu_pipe(scheduler):
    """the pipeline with stand-in modules on the CPU: everything up to the choice of the run path is host arithmetic"""
    import ladi_vton_amd as L

    class Pipe(L.StableDiffusionTryOnePipeline):
        _execution_device = torch.device("cpu")

        def _run_modular(self, *a, **k):
            raise _Recorded(k)
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=[8, 8, 8, 8], scaling_factor=0.18215))
    unet = SimpleNamespace(config=SimpleNamespace(sample_size=4))
    return Pipe(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=scheduler)


def _cpu_args(**kw):
    a = dict(image=torch.zeros(1, 3, 32, 32), mask_image=torch.zeros(1, 1, 32, 32), pose_map=torch.zeros(1, 18, 32, 32),
             warped_cloth=torch.zeros(1, 3, 32, 32), prompt_embeds=torch.zeros(1, 4, 8), negative_prompt_embeds=torch.zeros(1, 4, 8),
             height=32, width=32, num_inference_steps=8, output_type="np")
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,match", [
    (dict(preserve_unmasked="latent"), "preserve_unmasked"), (dict(preserve_unmasked=True), "preserve_unmasked"),
    (dict(preserve_unmasked=3), "preserve_unmasked"), (dict(preserve_unmasked=["pixels"]), "preserve_unmasked"),
    (dict(preserve_unmasked="pixels", mask_feather=-1.0), "mask_feather"), (dict(preserve_unmasked="both", mask_feather=32.5), "mask_feather"),
    (dict(preserve_unmasked="pixels", mask_feather=float("nan")), "mask_feather"), (dict(preserve_unmasked="pixels", mask_feather="wide"), "mask_feather"),
    (dict(preserve_unmasked="latents", mask_feather=2.0), "needs preserve_unmasked='pixels'"), (dict(mask_feather=2.0), "needs preserve_unmasked='pixels'"),
])
def test_pipeline_refuses_bad_preserve_arguments(kw, match):
    import ladi_vton_amd as L
    with pytest.raises(ValueError, match=match):
        _cpu_pipe(L.DDIMScheduler())(**_cpu_args(**kw))


@pytest.mark.parametrize("kw,want", [({}, (0, 0.0)), (dict(preserve_unmasked="latents"), (1, 0.0)), (dict(preserve_unmasked="pixels"), (2, 0.0)),
                                     (dict(preserve_unmasked="both", mask_feather=4), (3, 4.0)), (dict(preserve_unmasked="pixels", mask_feather=32), (2, 32.0))])
def test_pipeline_hands_the_mode_to_the_run(kw, want):
    import ladi_vton_amd as L
    with pytest.raises(_Recorded) as e:
        _cpu_pipe(L.DDIMScheduler())(**_cpu_args(**kw))
    assert e.value.args[0]["preserve"] == want


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def _loop_inputs(kind, n, B=2, h=4, w=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    s = SR.make_mirror(kind)
    s.set_timesteps(n)
    evals = len(s.timesteps)
    eps = torch.randn((evals, 2 * B, 4, h, w), generator=g, dtype=torch.float64)
    lat0 = torch.randn((B, 4, h, w), generator=g, dtype=torch.float64) * s.init_noise_sigma
    z0 = torch.randn((B, 4, h, w), generator=g, dtype=torch.float64)
    noise = torch.randn((B, 4, h, w), generator=g, dtype=torch.float64)
    table = [7.5 if i % 3 else 1.0 for i in range(evals)]
    return s, eps, table, lat0, z0, noise


@pytest.mark.parametrize("kind", list(KIND))
def test_reference_loop_with_nothing_to_keep_is_the_guidance_loop_exactly(kind):
    """an all-ones mask: no latent pixel is kept, and the loop is tests/guidance_ref.py sched_reference bit for bit"""
    s, eps, table, lat0, z0, noise = _loop_inputs(kind, 8)
    keep = R.keep_mask(torch.ones(2, 1, 32, 48))
    assert not keep.any()
    got = R.sched_reference(s, eps, table, 0.0, lat0, keep, z0, noise, generator=torch.Generator().manual_seed(9))
    s2 = SR.make_mirror(kind)
    s2.set_timesteps(8)
    want = G.sched_reference(s2, eps, table, 0.0, lat0, generator=torch.Generator().manual_seed(9))
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", list(KIND))
def test_reference_loop_with_everything_to_keep_ends_at_z0(kind):
    """an all-zeros mask: every evaluation leaves k_x z0 + k_n noise, the last one z0 itself"""
    s, eps, table, lat0, z0, noise = _loop_inputs(kind, 8)
    keep = R.keep_mask(torch.zeros(2, 1, 32, 48))
    assert keep.all()
    seen = []
    got = R.sched_reference(s, eps, table, 0.0, lat0, keep, z0, noise, generator=torch.Generator().manual_seed(9), seen=seen)
    assert torch.equal(got, z0)
    kc = R.keep_coeffs(s)
    for i, x in enumerate(seen[:-1]):
        assert torch.equal(x, kc[i][0] * z0 + kc[i][1] * noise), i


def test_keep_mask_needs_the_whole_footprint():
    """one masked pixel anywhere in an 8x8 footprint takes its latent pixel out of the keep set; the top-left nearest sample would miss it"""
    m = torch.zeros(1, 1, 16, 24)
    m[0, 0, 7, 15] = 0.6          # bottom-right corner of footprint (0, 1); binarised at 0.5
    m[0, 0, 8, 0] = 0.4           # below the threshold: not masked
    keep = R.keep_mask(m)
    want = torch.ones(1, 1, 2, 3, dtype=torch.bool)
    want[0, 0, 0, 1] = False
    assert torch.equal(keep, want)
    assert torch.nn.functional.interpolate(R.binarise(m), size=(2, 3)).sum() == 0


def test_feather_reference_properties():
    m = torch.zeros(1, 1, 16, 24)
    m[0, 0, :, 12:] = 1
    f = R.feather(m, 2.0)
    assert f.dtype == torch.float64 and f.shape == m.shape and float(f.min()) >= 0 and float(f.max()) <= 1 + 1e-15
    assert torch.allclose(f[0, 0, 0], f[0, 0, 15]) and abs(float(f[0, 0, 3, 11] + f[0, 0, 3, 12]) - 1.0) < 1e-12     # the edge is symmetric
    assert torch.allclose(R.feather(torch.ones(1, 1, 8, 8), 0.5), torch.ones(1, 1, 8, 8, dtype=torch.float64), atol=1e-15)
    w, r = R.feather_weights(4.0)
    assert r == 12 and len(w) == 25 and abs(float(w.sum()) - 1.0) < 1e-15


def test_modular_feather_agrees_with_the_reference_and_keeps_constants():
    """the torch fp32 blur of the modular path: within the device kernel's bound of the float64 reference, exactly 0 / 1 away from the edge"""
    from ladi_vton_amd.pipeline import feather_mask
    m = torch.zeros(2, 1, 32, 48)
    m[:, :, 5:20, 10:30] = 1
    m[1, :, :, :2] = 1
    for sigma in (0.5, 2.0):
        got, ref = feather_mask(m, sigma), R.feather(m, sigma)
        r = R.feather_weights(sigma)[1]
        assert got.dtype == torch.float32 and float((got.double() - ref).abs().max()) <= 4 * (2 * r + 2) * 2.0 ** -24
        assert (got[0, 0, 5 + r:20 - r, 10 + r:30 - r] == 1).all() and (got[0, 0, 20 + r:, :] == 0).all()
