"""Reference for starting the try-on loop from an image or latents (`strength`): the yardstick tests/test_cpu_strength.py and
tests/test_gpu_strength.py compare the library with.  The step arithmetic, the resample and the start latents are restated here in
float64; tests/ref_tryon.py's loop (init_latents=, first_step=) drives the oracle modules with the package's scheduler mirrors
(set_timesteps(n, first_step=)), whose tails tests/test_cpu_strength.py pins against the native tables.

    init_timestep = min(int(N * strength), N)        diffusers' get_timesteps, Python float64
    first_step    = N - init_timestep                the run is the evaluations of steps first_step .. of the N-step schedule
    resample      F.interpolate(mode="bilinear", align_corners=False): source coordinate max((o + 0.5) * in / out - 0.5, 0), lower
                  neighbour floor(src), upper one clamped to the last row / column, no antialias; equal sizes: the tensor itself
    x_start       = k_x * resample(init) + k_n * noise
                  DDIM / PNDM / DPM-Solver++: k_x = sqrt(a_t), k_n = sqrt(1 - a_t) at t = timesteps[first_step]
                  LMS / Euler / Euler-ancestral: k_x = 1, k_n = sigma[first_step]
                  init_is_noisy: k_x = 1, k_n = 0 (the init is the loop's latents at that step)
"""
import math

import torch
import torch.nn.functional as F

from oracle import pipeline as P

SCHEDULERS = ("ddim", "pndm", "lms", "dpmpp2m", "euler", "euler_a")
SIGMA_KINDS = ("lms", "euler", "euler_a")


def first_step_of(strength, n):
    init_timestep = min(int(n * float(strength)), n)
    return n - init_timestep


def _axis(n_in, n_out):
    """-> (i0, i1, lam) of every output index along one axis, float64"""
    o = torch.arange(n_out, dtype=torch.float64)
    src = ((o + 0.5) * n_in / n_out - 0.5).clamp(min=0.0)
    i0 = src.floor().clamp(max=n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.double()


def resample(x, h, w):
    """x [B, C, hs, ws] -> float64 [B, C, h, w]"""
    x = x.double()
    hs, ws = x.shape[2:]
    if (hs, ws) == (h, w):
        return x
    y0, y1, ly = _axis(hs, h)
    x0, x1, lx = _axis(ws, w)
    ly, lx = ly.view(1, 1, h, 1), lx.view(1, 1, 1, w)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


def start_latents(init, noise, k_x, k_n, h, w):
    """float64 [B, 4, h, w]; noise may be None when k_n == 0"""
    x = k_x * resample(init, h, w)
    return x if k_n == 0 else x + k_n * noise.double()


def make_mirror(name):
    import ladi_vton_amd as L
    return {"ddim": L.DDIMScheduler, "pndm": L.PNDMScheduler, "lms": L.LMSDiscreteScheduler, "dpmpp2m": L.DPMSolverMultistepScheduler,
            "euler": L.EulerDiscreteScheduler, "euler_a": L.EulerAncestralDiscreteScheduler}[name]()


def start_coeffs(name, sch):
    """(k_x, k_n) in float64 for a mirror `sch` whose set_timesteps(n, first_step=) is done"""
    if name in SIGMA_KINDS:
        return 1.0, float(sch.sigmas[0])
    a = float(P.alphas_cumprod()[int(sch.timesteps[0])].double())
    return math.sqrt(a), math.sqrt(1.0 - a)


def synthetic_init(B, hs, ws, seed=77):
    """smooth latents of the magnitude the tiny model's loop holds: a low-resolution field, upsampled, plus a little white noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((B, 4, max(hs // 4, 1), max(ws // 4, 1)), generator=g)
    x = F.interpolate(low, size=(hs, ws), mode="bilinear", align_corners=False)
    return (x + 0.1 * torch.randn((B, 4, hs, ws), generator=g)).float()
