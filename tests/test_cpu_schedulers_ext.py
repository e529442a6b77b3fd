"""DPM-Solver++ multistep, Euler and Euler-ancestral schedulers on the host (no GPU): the native step tables and the host mirrors
(ladi_vton_amd/schedulers.py) against the float64 restatement in tests/sched_ext_ref.py, plus known-answer anchors that do not depend
on that restatement."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pipeline as P
from tests import sched_ext_ref as R

DPM, EULER, EULER_A = 3, 4, 5
ORDER = lambda o: (o << 8)          # noqa: E731  (bits 8-9: solver_order)
HEUN, NO_LOF = 1 << 10, 1 << 11


def _code(order, solver_type, lof):
    return DPM | (ORDER(order) if order != 2 else 0) | (HEUN if solver_type == "heun" else 0) | (0 if lof else NO_LOF)


def _table(lib, code, n):
    ac = P.alphas_cumprod().contiguous()
    ts, rows = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))()
    cnt = lib.ladi_sched_table(code, n, ctypes.c_void_p(ac.data_ptr()), ts, rows, n + 2)
    assert cnt > 0, lib_error()
    return list(ts[:cnt]), np.array(list(rows[:10 * cnt]), dtype=np.float64).reshape(cnt, 10)


def lib_error():
    from ladi_vton_amd import _lib
    return _lib.last_error()


def _timesteps(lib, code, n):
    buf = (ctypes.c_int * (n + 2))()
    cnt = lib.ladi_sched_timesteps(code, n, buf, n + 2)
    return cnt, list(buf[:max(cnt, 0)])


@pytest.mark.parametrize("n", [7, 14, 15, 20, 25, 50, 100])
def test_dpm_timesteps_exact(lib, n):
    import ladi_vton_amd as L
    cnt, ts = _timesteps(lib, DPM, n)
    assert cnt == n and ts == R.dpm_timesteps(n)
    s = L.DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == ts
    if n == 50:
        assert ts[:3] == [999, 979, 959] and ts[-1] == 20
    assert _table(lib, DPM, n)[0] == [float(t) for t in ts]


def test_dpm_duplicate_timesteps_rejected(lib):
    import ladi_vton_amd as L
    assert R.dpm_timesteps(1000)[499:501] == [500, 500]          # diffusers 0.14 would fail in step() on these
    cnt, _ = _timesteps(lib, DPM, 1000)
    assert cnt < 0 and "duplicate" in lib_error()
    s = L.DPMSolverMultistepScheduler()
    with pytest.raises(L.NativeError, match="duplicate"):
        s.set_timesteps(1000)
    assert _timesteps(lib, DPM, 999)[0] == 999


@pytest.mark.parametrize("order,solver_type,lof", [(1, "midpoint", True), (2, "midpoint", True), (2, "heun", True), (3, "midpoint", True),
                                                   (2, "midpoint", False), (3, "heun", False)])
@pytest.mark.parametrize("n", [6, 14, 20])
def test_dpm_native_table_matches_restatement(lib, order, solver_type, lof, n):
    """x' = c_x x + c_e sum_k w_k m_k, m0 = p_x x + p_e eps: every coefficient vs the restatement's linear update (rtol 1e-5)"""
    ts, tb = _table(lib, _code(order, solver_type, lof), n)
    ref = R.RefDPM(order, solver_type, lof)
    ref.set_timesteps(n)
    assert len(ts) == n
    for i in range(n):
        c_x, c_e, w, p_x, p_e, c_n, isn = tb[i, 0], tb[i, 1], tb[i, 2:6], tb[i, 6], tb[i, 7], tb[i, 8], tb[i, 9]
        unit = [[1.0 if k == j else 0.0 for k in range(3)] for j in range(3)]
        want_x = ref.update(i, 1.0, [0.0, 0.0, 0.0])
        want_w = [ref.update(i, 0.0, unit[j]) for j in range(3)]
        s0 = ts[i]
        assert np.isclose(c_x, want_x, rtol=1e-5, atol=0), (i, c_x, want_x)
        assert np.allclose(c_e * w[:3], want_w, rtol=1e-5, atol=1e-7), (i, c_e * w[:3], want_w)
        assert w[3] == 0.0 and c_n == 0.0 and isn == 1.0
        assert np.isclose(p_x, 1.0 / ref.alpha(int(s0)), rtol=1e-6) and np.isclose(p_e, -ref.sigma(int(s0)) / ref.alpha(int(s0)), rtol=1e-6)
        eff = ref.step_order(i)
        assert not np.any(w[eff:3]), (i, eff, w)                 # the update uses exactly `eff` history entries
    if lof and n < 15:
        assert not np.any(tb[-1, 3:6]) and not np.any(tb[-2, 4:6])


@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("n", [5, 20, 50])
def test_euler_native_table_matches_restatement(lib, ancestral, n):
    ts, tb = _table(lib, EULER_A if ancestral else EULER, n)
    ref = R.RefEuler(ancestral)
    ref.set_timesteps(n)
    assert ts == ref.timesteps
    for i in range(n):
        ce, cn = ref.coeffs(i)
        assert tb[i, 0] == 1.0 and not tb[i, 3:8].any()
        assert np.isclose(tb[i, 1] * tb[i, 2], ce, rtol=1e-5, atol=0) and np.isclose(tb[i, 8], cn, rtol=1e-5, atol=0), (i, tb[i], ce, cn)
        want_isn = 1.0 / (float(ref.sigmas[i + 1]) ** 2 + 1) ** 0.5 if i + 1 < n else 1.0
        assert np.isclose(tb[i, 9], want_isn, rtol=1e-6)


def _eps_seq(n, shape, seed):
    g = np.random.default_rng(seed)
    return [g.standard_normal(shape) for _ in range(n)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("order,solver_type", [(1, "midpoint"), (2, "midpoint"), (2, "heun"), (3, "midpoint"), (3, "heun")])
@pytest.mark.parametrize("lof", [True, False])
@pytest.mark.parametrize("n", [8, 14, 15, 25])
def test_dpm_mirror_trajectory_matches_restatement(order, solver_type, lof, n):
    import ladi_vton_amd as L
    s = L.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type, lower_order_final=lof)
    ref = R.RefDPM(order, solver_type, lof)
    s.set_timesteps(n)
    ref.set_timesteps(n)
    assert s.init_noise_sigma == 1.0 and s.order == 1
    shape = (2, 4, 6, 5)
    eps = _eps_seq(n, shape, 100 + n + 10 * order)
    x0 = np.random.default_rng(7).standard_normal(shape)
    x, xr = torch.tensor(x0, dtype=torch.float32), x0.copy()
    for i, t in enumerate(s.timesteps):
        assert torch.equal(s.scale_model_input(x, t), x)
        x = s.step(torch.tensor(eps[i], dtype=torch.float32), t, x).prev_sample
        xr = ref.step(eps[i], int(t), xr)
        assert _rel(x.numpy(), xr) < 1e-5, (i, _rel(x.numpy(), xr))


@pytest.mark.parametrize("ancestral", [False, True])
def test_euler_mirror_trajectory_matches_restatement(ancestral):
    import ladi_vton_amd as L
    n, shape = 20, (2, 4, 6, 5)
    s = L.EulerAncestralDiscreteScheduler() if ancestral else L.EulerDiscreteScheduler()
    ref = R.RefEuler(ancestral)
    s.set_timesteps(n)
    ref.set_timesteps(n)
    assert s.timesteps.tolist() == ref.timesteps and abs(s.init_noise_sigma - ref.init_noise_sigma) < 1e-6
    eps = _eps_seq(n, shape, 3)
    x = torch.tensor(np.random.default_rng(4).standard_normal(shape) * s.init_noise_sigma, dtype=torch.float32)
    xr = x.double().numpy()
    g, gr = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    for i, t in enumerate(s.timesteps):
        xs = s.scale_model_input(x, t)
        assert _rel(xs.numpy(), ref.scale_model_input(x.double().numpy(), float(t))) < 1e-6
        x = s.step(torch.tensor(eps[i], dtype=torch.float32), t, x, generator=g).prev_sample
        noise = torch.randn(shape, generator=gr, dtype=torch.float32).double().numpy()   # one draw per step, also for Euler (unused)
        xr = ref.step(eps[i], float(t), xr, noise=noise)
        assert _rel(x.numpy(), xr) < 1e-5, (i, _rel(x.numpy(), xr))
    assert torch.equal(g.get_state(), gr.get_state())            # the generator is left where diffusers leaves it


def test_dpm_first_order_step_equals_ddim_step():
    """known answer: a first-order DPM-Solver++ step is exactly a DDIM (eta = 0) step between the same two timesteps"""
    import ladi_vton_amd as L
    n = 10
    s = L.DPMSolverMultistepScheduler(solver_order=1)
    s.set_timesteps(n)
    ac = s.alphas_cumprod.double()
    shape = (1, 4, 3, 3)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(shape, generator=g)
    for i in (0, 4, n - 1):
        t = int(s.timesteps[i])
        tp = 0 if i == n - 1 else int(s.timesteps[i + 1])
        e = torch.randn(shape, generator=g)
        s.set_timesteps(n)
        got = s.step(e, t, x).prev_sample.double()
        x0 = (x.double() - (1 - ac[t]).sqrt() * e.double()) / ac[t].sqrt()
        ddim = ac[tp].sqrt() * x0 + (1 - ac[tp]).sqrt() * e.double()
        assert float((got - ddim).norm() / ddim.norm()) < 1e-6, i


def test_euler_first_step_equals_lms_first_step(lib):
    import ladi_vton_amd as L
    n = 12
    e, l_ = L.EulerDiscreteScheduler(), L.LMSDiscreteScheduler()
    e.set_timesteps(n)
    l_.set_timesteps(n)
    g = torch.Generator().manual_seed(9)
    x, eps = torch.randn((2, 4, 5, 5), generator=g) * l_.init_noise_sigma, torch.randn((2, 4, 5, 5), generator=g)
    a = e.step(eps, e.timesteps[0], x).prev_sample
    b = l_.step(eps, l_.timesteps[0], x).prev_sample
    assert float((a - b).norm() / b.norm()) < 1e-6
    _, tb = _table(lib, EULER, n)
    assert abs(tb[0, 1] * tb[0, 2] - l_._coeffs[0][0]) <= 1e-5 * abs(l_._coeffs[0][0])


def test_euler_ancestral_step_into_sigma_zero_returns_data_prediction(lib):
    import ladi_vton_amd as L
    n = 9
    s = L.EulerAncestralDiscreteScheduler()
    s.set_timesteps(n)
    g = torch.Generator().manual_seed(5)
    x, eps = torch.randn((2, 4, 4, 4), generator=g), torch.randn((2, 4, 4, 4), generator=g)
    t = s.timesteps[-1]
    sigma = float(s.sigmas[n - 1])
    assert float(s.sigmas[n]) == 0.0
    got = s.step(eps, t, x, generator=torch.Generator().manual_seed(1)).prev_sample
    assert torch.allclose(got, x - sigma * eps, rtol=0, atol=1e-6)
    _, tb = _table(lib, EULER_A, n)
    assert tb[-1, 8] == 0.0 and np.isclose(tb[-1, 1] * tb[-1, 2], -sigma, rtol=1e-6)


@pytest.mark.parametrize("n", [5, 20, 50])
def test_euler_sigmas_and_timesteps_equal_lms(lib, n):
    import ladi_vton_amd as L
    ts, sg = (ctypes.c_double * n)(), (ctypes.c_float * (n + 1))()
    ac = P.alphas_cumprod().contiguous()
    assert lib.ladi_sched_lms(n, ctypes.c_void_p(ac.data_ptr()), ts, sg, None) == n
    for cls in (L.EulerDiscreteScheduler, L.EulerAncestralDiscreteScheduler):
        s, l_ = cls(), L.LMSDiscreteScheduler()
        assert s.init_noise_sigma == l_.init_noise_sigma
        s.set_timesteps(n)
        assert s.timesteps.dtype == torch.float64 and s.timesteps.tolist() == list(ts)
        assert s.sigmas.tolist() == list(sg) and s.init_noise_sigma == float(max(sg))
        x = torch.ones(1, 4, 2, 2)
        assert torch.equal(s.scale_model_input(x, s.timesteps[3]), x / ((float(sg[3]) ** 2 + 1) ** 0.5))
    for code in (EULER, EULER_A):
        assert _table(lib, code, n)[0] == list(ts)


@pytest.mark.parametrize("code", [6, 15, 16, 1 << 4, 1 << 7, -1, DPM | (1 << 12), DPM | (1 << 30), 0 | ORDER(1), 1 | HEUN,
                                  2 | NO_LOF, EULER | ORDER(3), EULER_A | HEUN])
def test_invalid_scheduler_codes_rejected(lib, code):
    cnt, _ = _timesteps(lib, code, 20)
    assert cnt < 0 and "scheduler" in lib_error(), (code, lib_error())
    assert _table_rc(lib, code, 20) < 0


def _table_rc(lib, code, n):
    rows = (ctypes.c_float * (10 * (n + 2)))()
    return lib.ladi_sched_table(code, n, None, None, rows, n + 2)


@pytest.mark.parametrize("code", [EULER, EULER_A, 2])
def test_fractional_kinds_refused_by_integer_timesteps(lib, code):
    cnt, _ = _timesteps(lib, code, 20)
    assert cnt < 0 and "fractional" in lib_error()


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("lof", [True, False])
def test_dpm_option_codes(lib, order, solver_type, lof):
    import ladi_vton_amd as L
    s = L.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type, lower_order_final=lof)
    assert s.kind == _code(order, solver_type, lof)
    assert _timesteps(lib, s.kind, 20) == (20, R.dpm_timesteps(20))
    assert _timesteps(lib, DPM | ORDER(order) | (HEUN if solver_type == "heun" else 0), 20)[0] == 20


def test_mirror_rejections():
    import ladi_vton_amd as L
    assert L.DPMSolverMultistepScheduler().kind == DPM                      # the diffusers defaults: DPM-Solver++ 2M, midpoint
    for kw in (dict(algorithm_type="dpmsolver"), dict(thresholding=True), dict(prediction_type="v_prediction"),
               dict(prediction_type="sample")):
        with pytest.raises(NotImplementedError):
            L.DPMSolverMultistepScheduler(**kw)
    for kw in (dict(solver_order=4), dict(solver_type="bh2")):
        with pytest.raises(ValueError):
            L.DPMSolverMultistepScheduler(**kw)
    s = L.EulerDiscreteScheduler()
    s.set_timesteps(10)
    with pytest.raises(NotImplementedError):
        s.step(torch.zeros(1, 4, 2, 2), s.timesteps[0], torch.zeros(1, 4, 2, 2), s_churn=0.5)


def test_ancestral_generator_list_draws_per_sample():
    """the repo's RNG rule (DDIMScheduler.step, eta > 0): a LIST of generators draws one [1, ...] tensor per sample"""
    import ladi_vton_amd as L
    n, shape = 6, (2, 4, 3, 3)
    s = L.EulerAncestralDiscreteScheduler()
    s.set_timesteps(n)
    x, eps = torch.zeros(shape), torch.zeros(shape)
    gens = [torch.Generator().manual_seed(40 + b) for b in range(2)]
    got = s.step(eps, s.timesteps[0], x, generator=gens).prev_sample
    s0, s1 = float(s.sigmas[0]), float(s.sigmas[1])
    up = (s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2) ** 0.5
    want = torch.cat([torch.randn((1,) + shape[1:], generator=torch.Generator().manual_seed(40 + b)) for b in range(2)]) * up
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        s.step(eps, s.timesteps[1], x, generator=gens[:1])
