"""Starting the loop at an intermediate step (`strength`) on the host, no GPU: the native tail tables (ladi_sched_table_from) against the
whole-run tables and against the scheduler mirrors' step(), the start coefficients against the mirrors' add_noise, the refusals, the step
arithmetic of tests/strength_ref.py against known diffusers answers, the restated resample against torch, and the pipeline's argument
validation.  Bounds: bit equality where a tail row is the whole run's row; otherwise those of tests/test_cpu_schedulers_ext.py for a table
against a mirror (coefficients rtol 1e-5, trajectories rel-L2 < 1e-5)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pipeline as P
from tests import strength_ref as R

DDIM, PNDM, LMS, DPM, EULER, EULER_A = 0, 1, 2, 3, 4, 5
KIND = {"ddim": DDIM, "pndm": PNDM, "lms": LMS, "dpmpp2m": DPM, "euler": EULER, "euler_a": EULER_A}
NS = [8, 50]


def lib_error():
    from ladi_vton_amd import _lib
    return _lib.last_error()


def _from(lib, code, n, first_step, eta=0.0):
    """-> (timesteps, rows float32 [evals, 10], start float32 [3]) or (rc, message)"""
    ac = P.alphas_cumprod().contiguous()
    ts, rows, start = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))(), (ctypes.c_float * 3)()
    cnt = lib.ladi_sched_table_from(code, n, ctypes.c_void_p(ac.data_ptr()), eta, first_step, ts, rows, n + 2, start)
    if cnt < 0:
        return cnt, lib_error()
    return list(ts[:cnt]), np.array(list(rows[:10 * cnt]), dtype=np.float32).reshape(cnt, 10), np.array(list(start), dtype=np.float32)


def _full(lib, code, n, eta=0.0):
    ac = P.alphas_cumprod().contiguous()
    ts, rows = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))()
    cnt = lib.ladi_sched_table_eta(code, n, ctypes.c_void_p(ac.data_ptr()), eta, ts, rows, n + 2)
    assert cnt > 0, lib_error()
    return list(ts[:cnt]), np.array(list(rows[:10 * cnt]), dtype=np.float32).reshape(cnt, 10)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_steps(n, kind):
    return sorted({1, n // 2, n - 2 if kind == "pndm" else n - 1})


# ------------------------------------------------------------------------------------------------------------------ tail tables
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", list(KIND))
def test_first_step_zero_is_the_whole_table_bitwise(lib, kind, n):
    for eta in ((0.0, 0.5) if kind == "ddim" else (0.0,)):
        ts, rows, start = _from(lib, KIND[kind], n, 0, eta)
        ts_f, rows_f = _full(lib, KIND[kind], n, eta)
        assert ts == ts_f and np.array_equal(_bits(rows), _bits(rows_f))
        s = R.make_mirror(kind)
        s.set_timesteps(n)
        assert start[0] == 0.0 and start[1] == np.float32(s.init_noise_sigma)
        want_scale0 = 1.0 / (float(s.sigmas[0]) ** 2 + 1.0) ** 0.5 if kind in R.SIGMA_KINDS else 1.0
        assert np.isclose(start[2], want_scale0, rtol=1e-6)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("ddim", 0.5), ("euler", 0.0), ("euler_a", 0.0)])
def test_single_step_kinds_tail_is_a_slice_bitwise(lib, kind, eta, n):
    ts_f, rows_f = _full(lib, KIND[kind], n, eta)
    for k in _first_steps(n, kind):
        ts, rows, _ = _from(lib, KIND[kind], n, k, eta)
        assert ts == ts_f[k:] and np.array_equal(_bits(rows), _bits(rows_f[k:])), k


@pytest.mark.parametrize("n", NS)
def test_lms_tail_warms_up_again(lib, n):
    """rows from first_step + 3 on are the whole run's; the first three are orders 1..3 (exactly that many weights), the first one Euler's"""
    ts_f, rows_f = _full(lib, LMS, n)
    _, rows_e = _full(lib, EULER, n)
    for k in _first_steps(n, "lms"):
        ts, rows, _ = _from(lib, LMS, n, k)
        assert ts == ts_f[k:] and len(rows) == n - k
        assert np.array_equal(_bits(rows[3:]), _bits(rows_f[k + 3:]))
        for j in range(min(3, n - k)):
            w = rows[j, 2:6]
            assert np.all(w[:j + 1] != 0) and not np.any(w[j + 1:]), (k, j, w)
            assert rows[j, 0] == 1.0 and rows[j, 1] == 1.0 and rows[j, 9] == rows_f[k + j, 9]
            assert np.isclose(w[:j + 1].sum(dtype=np.float64), float(rows_e[k + j, 1]), rtol=1e-5)     # weights integrate 1 over [sigma_i, sigma_i+1]
        assert np.isclose(rows[0, 2], rows_e[k, 1], rtol=1e-6)


@pytest.mark.parametrize("n", NS)
def test_dpm_tail_warms_up_again(lib, n):
    """DPM-Solver++ 2M: rows from first_step + 1 on are the whole run's, the first is first order: one weight, -alpha_t (e^-h - 1)"""
    ts_f, rows_f = _full(lib, DPM, n)
    ac = P.alphas_cumprod().double()
    for k in _first_steps(n, "dpmpp2m"):
        ts, rows, _ = _from(lib, DPM, n, k)
        assert ts == ts_f[k:]
        assert np.array_equal(_bits(rows[1:]), _bits(rows_f[k + 1:]))
        assert not np.any(rows[0, 3:6]) and rows[0, 2] != 0
        assert np.array_equal(_bits(rows[0, [0, 1, 6, 7, 8, 9]]), _bits(rows_f[k, [0, 1, 6, 7, 8, 9]]))
        s0, t = int(ts[0]), (int(ts[1]) if len(ts) > 1 else 0)
        lam = lambda u: float(0.5 * (ac[u].log() - (1 - ac[u]).log()))      # noqa: E731
        want = -float(ac[t].sqrt()) * np.expm1(-(lam(t) - lam(s0)))
        assert np.isclose(rows[0, 2], want, rtol=1e-5), (k, rows[0, 2], want)


@pytest.mark.parametrize("n", NS)
def test_pndm_tail_is_a_fresh_plms_run(lib, n):
    """a tail of m steps has m + 1 evaluations [u0, u1, u1, u2, ..] over the schedule's own step timesteps; every row is PNDMScheduler's
    transfer between the timesteps a fresh run over the tail visits, with the PLMS weights of an empty history"""
    ts_f, _ = _full(lib, PNDM, n)
    steps_f = [ts_f[0]] + ts_f[2:]
    ratio = 1000 // n
    ac = P.alphas_cumprod().double()
    weights = [[1.0], [0.5, 0.5], [1.5, -0.5], [23 / 12, -16 / 12, 5 / 12], [55 / 24, -59 / 24, 37 / 24, -9 / 24]]
    for k in _first_steps(n, "pndm"):
        ts, rows, _ = _from(lib, PNDM, n, k)
        u = steps_f[k:]
        m = n - k
        assert len(ts) == m + 1 and ts == [u[0], u[1], u[1]] + u[2:]
        s = R.make_mirror("pndm")
        s.set_timesteps(n, first_step=k)
        assert s.timesteps.tolist() == [int(t) for t in ts]
        for i in range(m + 1):
            t = int(ts[i])
            t, tp = (t + ratio, t) if i == 1 else (t, t - ratio)
            a_t, a_p = float(ac[t]), float(ac[tp] if tp >= 0 else ac[0])
            denom = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
            assert np.isclose(rows[i, 0], (a_p / a_t) ** 0.5, rtol=1e-5) and np.isclose(rows[i, 1], -(a_p - a_t) / denom, rtol=1e-5), (k, i)
            w = weights[min(i, 4)]
            assert np.allclose(rows[i, 2:2 + len(w)], w, rtol=1e-6) and not np.any(rows[i, 2 + len(w):6]), (k, i, rows[i])
            assert rows[i, 8] == 0.0 and rows[i, 9] == 1.0


# ------------------------------------------------------------------------------------------------------------------ table against mirror
def _simulate(kind, rows, eps, x, noise):
    """the step kernel's update in float64 from the 10-float rows: x' = c_x x + c_e sum_k w_k h_k + c_n noise, h_0 = eps (or the data
    prediction p_x x + p_e eps), earlier h from the history; PNDM's second evaluation starts from the first one's sample and pushes nothing"""
    hist, cur = [], None
    for i, r in enumerate(np.asarray(rows, dtype=np.float64)):
        c_x, c_e, w, p_x, p_e, c_n = r[0], r[1], r[2:6], r[6], r[7], r[8]
        second = kind == "pndm" and i == 1
        if kind == "pndm" and i == 0:
            cur = x
        xin = cur if second else x
        h0 = p_x * xin + p_e * eps[i] if kind == "dpmpp2m" else eps[i]
        hs = [h0] + hist
        acc = sum(w[j] * hs[j] for j in range(4) if w[j] != 0)
        if not second:
            hist = ([h0] + hist)[:3]
        x = c_x * xin + c_e * acc + c_n * noise[i]
    return x


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", list(KIND))
def test_tail_table_agrees_with_mirror(lib, kind, n, monkeypatch):
    """start_out against the mirror's add_noise coefficients, and the table's trajectory over a random eps sequence against the mirror's step()"""
    import ladi_vton_amd.schedulers as S
    shape = (2, 4, 6, 5)
    for k in _first_steps(n, kind):
        ts, rows, start = _from(lib, KIND[kind], n, k)
        s = R.make_mirror(kind)
        s.set_timesteps(n, first_step=k)
        assert [float(t) for t in s.timesteps.tolist()] == ts
        one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        k_x, k_n = float(s.add_noise(one, zero, s.timesteps[0])), float(s.add_noise(zero, one, s.timesteps[0]))
        assert np.isclose(start[0], k_x, rtol=1e-6) and np.isclose(start[1], k_n, rtol=1e-6), (k, start, k_x, k_n)
        assert (k_x, k_n) == pytest.approx(R.start_coeffs(kind, s), rel=1e-12)
        want_scale0 = 1.0 / (float(s.sigmas[0]) ** 2 + 1.0) ** 0.5 if kind in R.SIGMA_KINDS else 1.0
        assert np.isclose(start[2], want_scale0, rtol=1e-6)
        g = np.random.default_rng(1000 * n + 10 * k + KIND[kind])
        m = len(ts)
        eps = [g.standard_normal(shape) for _ in range(m)]
        noise = [g.standard_normal(shape) for _ in range(m)]
        draws = iter(noise)
        monkeypatch.setattr(S, "_step_noise", lambda shape, dtype, generator, device: torch.tensor(next(draws)).to(dtype))
        x0 = g.standard_normal(shape) * (k_x + k_n)
        x = torch.tensor(x0, dtype=torch.float32)
        for i, t in enumerate(s.timesteps):
            if i > 0 and kind in R.SIGMA_KINDS:
                want = 1.0 / (float(s.sigmas[i]) ** 2 + 1.0) ** 0.5
                assert np.isclose(rows[i - 1, 9], want, rtol=1e-6)
            x = s.step(torch.tensor(eps[i], dtype=torch.float32), t, x).prev_sample
        got = _simulate(kind, rows, eps, x0.astype(np.float32).astype(np.float64), noise)
        rel = float(np.linalg.norm(got - x.double().numpy()) / np.linalg.norm(got))
        assert rel < 1e-5, (kind, n, k, rel)


@pytest.mark.parametrize("order,solver_type,lof", [(3, "midpoint", True), (2, "heun", False), (1, "midpoint", True)])
def test_dpm_options_tail_agrees_with_mirror(lib, order, solver_type, lof):
    """the other solver orders / types: n = 8 < 15, so lower_order_final acts at the end of the tail, where it does in the whole run"""
    import ladi_vton_amd as L
    n, shape = 8, (2, 4, 6, 5)
    for k in (1, 4, 6, 7):
        s = L.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type, lower_order_final=lof)
        s.set_timesteps(n, first_step=k)
        ts, rows, _ = _from(lib, s.kind, n, k)
        _, rows_f = _full(lib, s.kind, n)
        assert np.array_equal(_bits(rows[order - 1:]), _bits(rows_f[k + order - 1:]))
        g = np.random.default_rng(k)
        eps = [g.standard_normal(shape) for _ in ts]
        x0 = g.standard_normal(shape).astype(np.float32)
        x = torch.tensor(x0)
        for i, t in enumerate(s.timesteps):
            x = s.step(torch.tensor(eps[i], dtype=torch.float32), t, x).prev_sample
        got = _simulate("dpmpp2m", rows, eps, x0.astype(np.float64), [0.0] * len(ts))
        assert float(np.linalg.norm(got - x.double().numpy()) / np.linalg.norm(got)) < 1e-5, k


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", list(KIND))
def test_first_step_out_of_range_is_refused(lib, kind, n):
    last = n - 2 if kind == "pndm" else n - 1
    assert not isinstance(_from(lib, KIND[kind], n, last)[0], int)
    for bad in (last + 1, n, n + 5, -1):
        rc, msg = _from(lib, KIND[kind], n, bad)
        assert rc < 0 and "first_step" in msg and "out of range" in msg, (bad, msg)
        with pytest.raises(ValueError, match="first_step"):
            R.make_mirror(kind).set_timesteps(n, first_step=bad)
    if kind == "pndm":
        assert "PNDM tail needs at least 2 steps" in _from(lib, PNDM, n, n - 1)[1]
    assert not isinstance(_from(lib, KIND[kind], n, last)[0], int)          # and the helper works afterwards


def test_mirror_defaults_are_unchanged():
    for kind in KIND:
        a, b = R.make_mirror(kind), R.make_mirror(kind)
        a.set_timesteps(10)
        b.set_timesteps(10, None, 0)
        assert torch.equal(a.timesteps, b.timesteps) and a.init_noise_sigma == b.init_noise_sigma
        if kind in R.SIGMA_KINDS:
            assert torch.equal(a.sigmas, b.sigmas) and len(a.sigmas) == 11
            c = R.make_mirror(kind)
            c.set_timesteps(10, first_step=4)
            assert torch.equal(c.sigmas, a.sigmas[4:]) and c.init_noise_sigma == a.init_noise_sigma


# ------------------------------------------------------------------------------------------------------------------ step arithmetic, resample
@pytest.mark.parametrize("n,strength,want", [(50, 0.3, 35), (10, 0.7, 3), (100, 0.29, 72), (8, 0.5, 4), (8, 1.0, 0), (50, 0.02, 49)])
def test_first_step_of_is_the_diffusers_arithmetic(n, strength, want):
    import ladi_vton_amd as L
    assert R.first_step_of(strength, n) == want
    assert L.strength_first_step(strength, n) == want


@pytest.mark.parametrize("src,dst", [((8, 12), (8, 12)), ((4, 6), (8, 12)), ((5, 7), (9, 13)), ((16, 24), (9, 13)), ((1, 1), (8, 12)),
                                     ((16, 12), (32, 24))])
def test_restated_resample_is_torch_bilinear(src, dst):
    """the float64 restatement against torch's fp32 F.interpolate(mode="bilinear", align_corners=False); equal sizes are bit-equal.  Bound:
    torch computes the source coordinate in fp32 (scale, product, subtraction: three roundings of a value up to the source side, 24 here), so
    a weight is off by up to 3 * 24 * 2^-24 = 4.3e-6, which moves the result by that times the neighbours' difference (sqrt(2) of the rms for
    white noise), on two axes: rel-L2 <= 2 * 4.3e-6 * sqrt(2) = 1.2e-5 in the worst case; 1e-5 is asserted (measured: below 1e-6)"""
    x = torch.randn((2, 4) + src, generator=torch.Generator().manual_seed(src[0] * 100 + dst[1]))
    got = R.resample(x, *dst)
    if src == dst:
        assert torch.equal(got, x.double())
        return
    want = F.interpolate(x, size=dst, mode="bilinear", align_corners=False).double()
    assert float((got - want).norm() / want.norm()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------ pipeline arguments
class _Recorded(Exception):
    pass


def _cpu_pipe(scheduler):
    """the pipeline with stand-in modules on the CPU: everything up to the choice of the run path is host arithmetic"""
    import ladi_vton_amd as L

    class Pipe(L.StableDiffusionTryOnePipeline):
        _execution_device = torch.device("cpu")

        def _prepare_init(self, *a, **k):
            raise AssertionError("the init was prepared although it is ignored")

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
    (dict(strength=-0.1), "strength"), (dict(strength=1.5), "strength"), (dict(strength=float("nan")), "strength"),
    (dict(strength=float("inf")), "strength"), (dict(strength=0.0), "no step"), (dict(strength=0.1), "no step"),       # int(8 * 0.1) = 0
    (dict(strength=0.5), "init_image` or `init_latents"),
    (dict(strength=0.5, init_image=torch.zeros(1, 3, 32, 32), init_latents=torch.zeros(1, 4, 4, 4)), "both"),
    (dict(strength=1.0, init_image=torch.zeros(1, 3, 32, 32), init_latents=torch.zeros(1, 4, 4, 4)), "both"),
])
def test_pipeline_refuses_bad_strength_arguments(kw, match):
    import ladi_vton_amd as L
    with pytest.raises(ValueError, match=match):
        _cpu_pipe(L.DDIMScheduler())(**_cpu_args(**kw))


def test_pipeline_refuses_a_pndm_tail_of_one_step():
    import ladi_vton_amd as L
    with pytest.raises(ValueError, match="PNDM tail needs at least 2 steps"):
        _cpu_pipe(L.PNDMScheduler())(**_cpu_args(strength=0.125, init_latents=torch.zeros(1, 4, 4, 4)))


def test_strength_one_with_an_init_takes_the_no_init_path():
    import ladi_vton_amd as L
    for kw in (dict(init_latents=torch.zeros(1, 4, 4, 4)), dict(init_image=torch.zeros(1, 3, 32, 32)), {}):
        with pytest.raises(_Recorded) as e:
            _cpu_pipe(L.DDIMScheduler())(**_cpu_args(strength=1.0, **kw))
        assert e.value.args[0]["init_latents"] is None and e.value.args[0]["first_step"] == 0


def test_strength_below_one_hands_the_tail_to_the_run():
    """first_step, the init and the tail's guidance schedule length reach the run path; a schedule of the whole run's length is refused"""
    import ladi_vton_amd as L
    init = torch.arange(64, dtype=torch.float32).view(1, 4, 4, 4)

    class Pipe(type(_cpu_pipe(L.DDIMScheduler()))):
        _prepare_init = L.StableDiffusionTryOnePipeline._prepare_init
    p = _cpu_pipe(L.DDIMScheduler())
    p.__class__ = Pipe
    with pytest.raises(_Recorded) as e:
        p(**_cpu_args(strength=0.5, init_latents=init, init_is_noisy=True, guidance_scale=[7.5] * 4))
    k = e.value.args[0]
    assert k["first_step"] == 4 and k["init_is_noisy"] is True and torch.equal(k["init_latents"], init) and k["guidance_table"] == [7.5] * 4
    assert p.scheduler.timesteps.tolist() == [376, 251, 126, 1]
    with pytest.raises(ValueError, match="8 entries but the scheduler runs 4 evaluations"):
        p(**_cpu_args(strength=0.5, init_latents=init, guidance_scale=[7.5] * 8))
    with pytest.raises(ValueError, match="init_latents"):
        p(**_cpu_args(strength=0.5, init_latents=torch.zeros(2, 4, 4, 4)))
