"""Test-local float64 restatement of diffusers 0.14 DDIMScheduler.step with eta (steps_offset 1, set_alpha_to_one False, clip_sample False,
epsilon prediction), independent of ladi_vton_amd/schedulers.py and of the native table builder:

    std  = eta * sqrt(max((1 - a_p) / (1 - a_t) * (1 - a_t / a_p), 0))
    x'   = sqrt(a_p) * (x - sqrt(1 - a_t) eps) / sqrt(a_t) + sqrt(max(1 - a_p - std^2, 0)) * eps + std * noise"""
import math

from oracle import pipeline as P


def timesteps(n):
    ratio = 1000 // n
    return [i * ratio + 1 for i in range(n)][::-1]


def coeffs(n, i, eta):
    """(c_x, c_e, c_n) of evaluation i: x' = c_x x + c_e eps + c_n noise, in float64"""
    ac = P.alphas_cumprod().double().numpy()
    t = timesteps(n)[i]
    tp = t - 1000 // n
    a_t, a_p = float(ac[t]), float(ac[tp]) if tp >= 0 else float(ac[0])
    std = eta * math.sqrt(max((1 - a_p) / (1 - a_t) * (1 - a_t / a_p), 0.0))
    c_x = math.sqrt(a_p / a_t)
    c_e = math.sqrt(max(1 - a_p - std * std, 0.0)) - math.sqrt(a_p) * math.sqrt(1 - a_t) / math.sqrt(a_t)
    return c_x, c_e, std


def step(n, i, eta, x, eps, noise):
    c_x, c_e, c_n = coeffs(n, i, eta)
    return c_x * x + c_e * eps + c_n * noise
