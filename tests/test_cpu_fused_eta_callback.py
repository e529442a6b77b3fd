"""DDIM with eta > 0 on the host (no GPU): the native step table (ladi_sched_table_eta) against the float64 restatement in
tests/ddim_eta_ref.py, eta = 0 rows identical to ladi_sched_table's, and the argument checks of the new entry points that need no device."""
import ctypes
import math

import numpy as np
import pytest

from ladi_vton_amd import _lib
from oracle import pipeline as P
from tests import ddim_eta_ref as R

DDIM, PNDM, LMS, DPM, EULER, EULER_A = 0, 1, 2, 3, 4, 5


def _table(lib, code, n, eta=None):
    ac = P.alphas_cumprod().contiguous()
    ts, rows = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))()
    if eta is None:
        cnt = lib.ladi_sched_table(code, n, ctypes.c_void_p(ac.data_ptr()), ts, rows, n + 2)
    else:
        cnt = lib.ladi_sched_table_eta(code, n, ctypes.c_void_p(ac.data_ptr()), eta, ts, rows, n + 2)
    assert cnt > 0, _lib.last_error()
    return list(ts[:cnt]), np.array(list(rows[:10 * cnt]), dtype=np.float32).reshape(cnt, 10)


@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [10, 50])
def test_ddim_eta_table_matches_restatement(lib, n, eta):
    """c_x, c_e * w0 and c_n of every row vs float64 diffusers DDIM, to fp32 rounding"""
    ts, tb = _table(lib, DDIM, n, eta)
    assert ts == [float(t) for t in R.timesteps(n)]
    for i in range(n):
        c_x, c_e, c_n = R.coeffs(n, i, eta)
        row = tb[i].astype(np.float64)
        assert row[2] == 1.0 and not row[3:8].any() and row[9] == 1.0, row
        assert math.isclose(row[0], c_x, rel_tol=2e-7), (i, row[0], c_x)
        assert math.isclose(row[1] * row[2], c_e, rel_tol=1e-6, abs_tol=1e-7), (i, row[1], c_e)
        assert math.isclose(row[8], c_n, rel_tol=2e-7, abs_tol=0), (i, row[8], c_n)
        assert (row[8] > 0) == (eta > 0)


@pytest.mark.parametrize("n", [10, 50])
def test_ddim_eta_zero_rows_bit_identical(lib, n):
    ts0, tb0 = _table(lib, DDIM, n)
    ts1, tb1 = _table(lib, DDIM, n, 0.0)
    assert ts0 == ts1
    assert tb0.tobytes() == tb1.tobytes()


def test_ddim_eta_one_keeps_eps_direction_real(lib):
    """eta = 1: 1 - a_p - std^2 stays >= 0 along the whole schedule (the max(., 0) never clips a real value to a different one)"""
    _, tb = _table(lib, DDIM, 50, 1.0)
    assert np.all(np.isfinite(tb))


@pytest.mark.parametrize("code", [PNDM, LMS, DPM, EULER, EULER_A])
def test_eta_rejected_for_other_schedulers(lib, code):
    """only DDIM takes eta: a non-zero one with any other scheduler code is an error, eta = 0 gives the plain table"""
    ac = P.alphas_cumprod().contiguous()
    rows = (ctypes.c_float * (10 * 64))()
    assert lib.ladi_sched_table_eta(code, 20, ctypes.c_void_p(ac.data_ptr()), 0.5, None, rows, 64) < 0
    assert "DDIM only" in _lib.last_error()
    _, a = _table(lib, code, 20)
    _, b = _table(lib, code, 20, 0.0)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("eta", [-0.1, float("nan"), float("inf")])
def test_eta_must_be_finite_non_negative(lib, eta):
    rows = (ctypes.c_float * (10 * 64))()
    assert lib.ladi_sched_table_eta(DDIM, 20, None, eta, None, rows, 64) < 0
    assert "eta" in _lib.last_error()


def test_handle_setters_reject_null(lib):
    assert lib.ladi_tryon_set_eta(None, 0.5) < 0
    assert lib.ladi_tryon_set_step_callback(None, _lib.NO_STEP_CALLBACK, None, 1, None) < 0


def test_mirror_ddim_eta_step_matches_restatement():
    """the host mirror (modular path) with an explicit variance_noise against the same restatement"""
    import torch
    import ladi_vton_amd as L
    s = L.DDIMScheduler()
    n, eta = 10, 0.7
    s.set_timesteps(n)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 5, 6), generator=g, dtype=torch.float64)
    for i, t in enumerate(s.timesteps):
        eps, nz = torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
        want = R.step(n, i, eta, x, eps, nz)
        got = s.step(eps, t, x, eta=eta, variance_noise=nz).prev_sample
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), i
        x = want


def test_null_step_callback_is_null():
    assert not _lib.NO_STEP_CALLBACK
    assert ctypes.cast(_lib.NO_STEP_CALLBACK, ctypes.c_void_p).value is None
