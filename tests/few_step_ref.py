"""Test-local float64 restatement of few-step sampling: the LCM and TCD updates and trailing timestep spacing for DDIM, Euler and
Euler-ancestral (SD2-inpainting config: scaled_linear 0.00085-0.012, 1000 training steps, epsilon prediction), written from the published
algorithms as a step-by-step recurrence and independent of ladi_vton_amd and of the native table builder.  Like the other schedulers'
restatements it is not pinned against diffusers itself.

step() is plain arithmetic with Python floats, so it runs on float64 numpy arrays (CPU tests) and on torch tensors (the oracle pipeline,
whose scheduler interface it follows: set_timesteps(n), timesteps, init_noise_sigma, scale_model_input(x, t), step(eps, t, x) -> x).
Stochastic updates take their noise from `noise_fn(shape)`, one call per drawing step, or from step(..., noise=)."""
import math

import numpy as np

from oracle import pipeline as P

T = 1000


def alphas_cumprod64():
    return P.alphas_cumprod().double().numpy()


def lcm_timesteps(n, original_steps=50):
    """the distilled model's grid arange(1, O + 1) * (T // O) - 1, reversed, sampled at floor(linspace(0, O, n, endpoint=False))"""
    grid = (np.arange(1, original_steps + 1) * (T // original_steps) - 1)[::-1]
    idx = np.floor(np.linspace(0, original_steps, num=n, endpoint=False)).astype(np.int64)
    return [int(t) for t in grid[idx]]


def trailing_timesteps(n):
    """t_i = round_half_even(T - i * (T / n)) - 1 (Python's round() rounds half to even)"""
    return [int(round(T - i * (T / n))) - 1 for i in range(n)]


class _Ref:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, noise_fn=None):
        self.noise_fn = noise_fn
        self.ac = alphas_cumprod64()

    def scale_model_input(self, x, t):
        return x

    def _noise(self, x, noise):
        return noise if noise is not None else self.noise_fn(tuple(x.shape))

    def x0(self, eps, t, x):
        a = float(self.ac[t])
        return (x - math.sqrt(1.0 - a) * eps) / math.sqrt(a)

    def add_noise(self, x0, noise, t):
        a = float(self.ac[int(t)])
        return math.sqrt(a) * x0 + math.sqrt(1.0 - a) * noise


class RefLCM(_Ref):
    """latent consistency model sampling: the boundary-condition mix of the data prediction, re-noised to the next timestep"""

    def __init__(self, original_steps=50, noise_fn=None):
        super().__init__(noise_fn)
        self.original_steps = original_steps

    def set_timesteps(self, n, first_step=0):
        self.timesteps = lcm_timesteps(n, self.original_steps)[first_step:]

    def step(self, eps, t, x, noise=None):
        t = int(t)
        i = self.timesteps.index(t)
        s = 10.0 * t                                             # timestep_scaling 10, sigma_data 0.5
        c_skip = 0.5 ** 2 / (s ** 2 + 0.5 ** 2)
        c_out = s / math.sqrt(s ** 2 + 0.5 ** 2)
        den = c_out * self.x0(eps, t, x) + c_skip * x
        if i == len(self.timesteps) - 1:
            return den
        return self.add_noise(den, self._noise(x, noise), self.timesteps[i + 1])


class RefTCD(_Ref):
    """trajectory consistency distillation sampling with stochasticity gamma"""

    def __init__(self, gamma=0.3, original_steps=50, noise_fn=None):
        super().__init__(noise_fn)
        self.gamma, self.original_steps = float(gamma), original_steps

    def set_timesteps(self, n, first_step=0):
        self.timesteps = lcm_timesteps(n, self.original_steps)[first_step:]

    def step(self, eps, t, x, noise=None):
        t = int(t)
        i = self.timesteps.index(t)
        last = i == len(self.timesteps) - 1
        t_prev = 0 if last else self.timesteps[i + 1]
        t_s = int(math.floor((1.0 - self.gamma) * t_prev))
        a_s, a_prev = float(self.ac[t_s]), float(self.ac[t_prev])
        x_s = math.sqrt(a_s) * self.x0(eps, t, x) + math.sqrt(1.0 - a_s) * eps
        if self.gamma > 0.0 and not last:
            return math.sqrt(a_prev / a_s) * x_s + math.sqrt(1.0 - a_prev / a_s) * self._noise(x, noise)
        return x_s


class RefDDIM(_Ref):
    """DDIM with eta; trailing=True: the trailing timesteps with prev = t - T // n, else the leading ones (steps_offset 1)"""

    def __init__(self, eta=0.0, trailing=True, noise_fn=None):
        super().__init__(noise_fn)
        self.eta, self.trailing = float(eta), trailing

    def set_timesteps(self, n, first_step=0):
        self.ratio = T // n
        ts = trailing_timesteps(n) if self.trailing else [i * self.ratio + 1 for i in range(n)][::-1]
        self.timesteps = ts[first_step:]

    def step(self, eps, t, x, noise=None):
        t = int(t)
        tp = t - self.ratio
        a_t, a_p = float(self.ac[t]), float(self.ac[tp] if tp >= 0 else self.ac[0])       # set_alpha_to_one = False
        std = self.eta * math.sqrt(max((1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p), 0.0))
        out = math.sqrt(a_p) * self.x0(eps, t, x) + math.sqrt(max(1.0 - a_p - std * std, 0.0)) * eps
        if self.eta > 0.0:
            out = out + std * self._noise(x, noise)
        return out


class RefEuler(_Ref):
    """Euler (s_churn = 0) and, with ancestral=True, Euler-ancestral over trailing timesteps: sigma = sqrt((1 - a) / a) at the integer
    timesteps, held in fp32, trailing 0"""

    def __init__(self, ancestral=False, noise_fn=None):
        super().__init__(noise_fn)
        self.ancestral = ancestral

    def set_timesteps(self, n, first_step=0):
        ts = trailing_timesteps(n)
        sig = np.array([math.sqrt((1.0 - float(self.ac[t])) / float(self.ac[t])) for t in ts] + [0.0]).astype(np.float32)
        self.init_noise_sigma = float(sig.max())
        self.timesteps, self.sigmas = [float(t) for t in ts][first_step:], sig[first_step:]

    def scale_model_input(self, x, t):
        i = self.timesteps.index(float(t))
        return x / ((float(self.sigmas[i]) ** 2 + 1) ** 0.5)

    def add_noise(self, x0, noise, t):
        return x0 + float(self.sigmas[self.timesteps.index(float(t))]) * noise

    def step(self, eps, t, x, noise=None):
        i = self.timesteps.index(float(t))
        s0, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if not self.ancestral:
            return x + (s1 - s0) * eps
        up = math.sqrt(s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2)
        down = math.sqrt(max(s1 ** 2 - up ** 2, 0.0))
        out = x + (down - s0) * eps
        # (Euler-ancestral draws at every step, the last included, where sigma_up = 0)
        return out + up * self._noise(x, noise)


def row_of(ref, i, probe_shape=(1,)):
    """-> (c_x, c_e, c_n) of the reference's update at evaluation i, recovered from its linearity in (x, eps, noise)"""
    t = ref.timesteps[i]
    z, one = np.zeros(probe_shape), np.ones(probe_shape)
    c_x = float(ref.step(z, t, one, noise=z)[0])
    c_e = float(ref.step(one, t, z, noise=z)[0])
    c_n = float(ref.step(z, t, z, noise=one)[0])
    return c_x, c_e, c_n


def keep_coeffs(ref):
    """the latent blend's rule: add_noise's coefficients at timesteps[i + 1], {1, 0} after the last evaluation"""
    out = []
    for i in range(len(ref.timesteps)):
        if i + 1 == len(ref.timesteps):
            out.append((1.0, 0.0))
        else:
            t = ref.timesteps[i + 1]
            out.append((float(ref.add_noise(1.0, 0.0, t)), float(ref.add_noise(0.0, 1.0, t))))
    return out
