"""Test-local float64 restatement of the DPM-Solver++ multistep, Euler and Euler-ancestral schedulers (diffusers 0.14.0 with the
SD2-inpainting config: scaled_linear 0.00085-0.012, 1000 training steps, epsilon prediction), written from the published formulas and
independent of ladi_vton_amd/schedulers.py and of the native table builder.  Like the other schedulers' restatements it is not pinned
against diffusers itself (not installable here).

step() is plain arithmetic with Python floats, so it runs on float64 numpy arrays (CPU tests) and on torch tensors (the oracle pipeline,
whose scheduler interface it follows: set_timesteps(n), timesteps, init_noise_sigma, scale_model_input(x, t), step(eps, t, x) -> x)."""
import math

import numpy as np

from oracle import pipeline as P


def alphas_cumprod64():
    return P.alphas_cumprod().double().numpy()


def dpm_timesteps(n):
    """linspace(0, 999, n + 1).round()[::-1][:-1] (numpy rounds half to even)"""
    return [int(v) for v in np.linspace(0, 999, n + 1).round()[::-1][:-1]]


def lms_sigmas(n):
    """timesteps linspace(0, 999, n)[::-1] (float64), sigmas interp(t, arange, sqrt((1 - a) / a)) of the fp32 table, held in fp32, trailing 0"""
    ac = P.alphas_cumprod()
    ts = np.linspace(0, 999, n, dtype=float)[::-1].copy()
    sig = (((1 - ac) / ac) ** 0.5).numpy()
    sig = np.interp(ts, np.arange(0, len(sig)), sig)
    return [float(t) for t in ts], np.concatenate([sig, [0.0]]).astype(np.float32)


class RefDPM:
    """DPMSolverMultistepScheduler(algorithm_type="dpmsolver++")"""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, solver_order=2, solver_type="midpoint", lower_order_final=True):
        self.solver_order, self.solver_type, self.lower_order_final = solver_order, solver_type, lower_order_final
        self.ac = alphas_cumprod64()

    def alpha(self, t):
        return math.sqrt(self.ac[t])

    def sigma(self, t):
        return math.sqrt(1.0 - self.ac[t])

    def lam(self, t):
        return math.log(self.alpha(t)) - math.log(self.sigma(t))

    def set_timesteps(self, n):
        self.n = n
        self.timesteps = dpm_timesteps(n)
        self.ms = []

    def scale_model_input(self, x, t):
        return x

    def step_order(self, i):
        order = min(self.solver_order, i + 1)                   # warm-up: one / two history entries
        if self.lower_order_final and self.n < 15:
            if i == self.n - 1:
                order = 1
            elif i == self.n - 2:
                order = min(order, 2)
        return order

    def update(self, i, x, ms):
        """x_t from x and the data predictions ms = [m0 (this step), m1, m2]"""
        ts = self.timesteps
        s0 = ts[i]
        t = 0 if i == self.n - 1 else ts[i + 1]
        order = self.step_order(i)
        a_t, h = self.alpha(t), self.lam(t) - self.lam(s0)
        em = math.exp(-h) - 1.0
        out = (self.sigma(t) / self.sigma(s0)) * x - a_t * em * ms[0]
        if order == 2:
            r0 = (self.lam(s0) - self.lam(ts[i - 1])) / h
            d1 = (ms[0] - ms[1]) / r0
            if self.solver_type == "midpoint":
                out = out - 0.5 * a_t * em * d1
            else:
                out = out + a_t * (em / h + 1.0) * d1
        elif order == 3:
            r0 = (self.lam(s0) - self.lam(ts[i - 1])) / h
            r1 = (self.lam(ts[i - 1]) - self.lam(ts[i - 2])) / h
            d1_0, d1_1 = (ms[0] - ms[1]) / r0, (ms[1] - ms[2]) / r1
            d1 = d1_0 + r0 / (r0 + r1) * (d1_0 - d1_1)
            d2 = (d1_0 - d1_1) / (r0 + r1)
            out = out + a_t * (em / h + 1.0) * d1 - a_t * ((em + h) / (h * h) - 0.5) * d2
        return out

    def step(self, eps, t, x):
        i = self.timesteps.index(int(t))
        s0 = self.timesteps[i]
        self.ms.append((x - self.sigma(s0) * eps) / self.alpha(s0))
        ms = list(reversed(self.ms[-3:])) + [None] * 3
        return self.update(i, x, ms)


class RefEuler:
    """EulerDiscreteScheduler (s_churn = 0) and, with ancestral=True, EulerAncestralDiscreteScheduler; the ancestral noise comes from
    `noise_fn(shape)` (one draw per step)"""
    order = 1

    def __init__(self, ancestral=False, noise_fn=None):
        self.ancestral, self.noise_fn = ancestral, noise_fn

    def set_timesteps(self, n):
        self.timesteps, self.sigmas = lms_sigmas(n)
        self.init_noise_sigma = float(self.sigmas.max())

    def scale_model_input(self, x, t):
        i = self.timesteps.index(float(t))
        return x / ((float(self.sigmas[i]) ** 2 + 1) ** 0.5)

    def coeffs(self, i):
        """(eps coefficient, noise coefficient) of step i"""
        s0, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if not self.ancestral:
            return s1 - s0, 0.0
        up = math.sqrt(s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2)
        down = math.sqrt(max(s1 ** 2 - up ** 2, 0.0))
        return down - s0, up

    def step(self, eps, t, x, noise=None):
        i = self.timesteps.index(float(t))
        ce, cn = self.coeffs(i)
        out = x + ce * eps
        if self.ancestral:
            if noise is None:
                noise = self.noise_fn(tuple(x.shape))
            out = out + cn * noise
        return out
