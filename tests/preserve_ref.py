"""Reference for keeping the unmasked region (`preserve_unmasked`): the yardstick tests/test_cpu_preserve.py and tests/test_gpu_preserve.py
compare the library with.  float64 torch for the blend coefficients, the feathered mask and the composite; tests/ref_tryon.py's loop
(preserve=) applies the blend after every scheduler step and the composite after the decode.

    keep      = 1 - max_pool2d(binarised mask, 8)            a latent pixel whose whole 8x8 footprint is unmasked
    z0        = scaling_factor * mean(vae.encode(image))     the posterior mode of the full, unmasked image (no RNG draw)
    after the scheduler update of evaluation i (the latents then belong to timesteps[i + 1]):
        latents[keep] = k_x[i] z0 + k_n[i] noise             the scheduler's add_noise at timesteps[i + 1], noise = the initial-latents noise
        latents[keep] = z0                                   after the last evaluation
    the blend acts on scheduler.step(...).prev_sample only: scheduler state (PLMS cur_sample, the eps / data-prediction history) is not blended
    pixels:   out = M g + (1 - M) p, g = clamp(decoded / 2 + 0.5, 0, 1), p = clamp(image / 2 + 0.5, 0, 1), M the binarised mask or its separable
              Gaussian blur (radius ceil(3 sigma), weights normalised in float64, replicate border); M == 0 / 1 select p / g
"""
import math

import torch
import torch.nn.functional as F

from tests import guidance_ref as G
from tests import strength_ref as SR

SCHEDULERS = SR.SCHEDULERS
MODES = {None: 0, "latents": 1, "pixels": 2, "both": 3}


def keep_coeffs(sch):
    """float64 [(k_x, k_n)] * evals for a mirror `sch` with set_timesteps done: add_noise's coefficients at timesteps[i + 1], read off the
    mirror's own add_noise (x0 = 1, noise = 0 and the reverse); the last row is (1, 0)"""
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    n = len(sch.timesteps)
    out = []
    for i in range(n):
        if i + 1 < n:
            t = sch.timesteps[i + 1]
            out.append((float(sch.add_noise(one, zero, t)), float(sch.add_noise(zero, one, t))))
        else:
            out.append((1.0, 0.0))
    return out


def binarise(mask):
    return (mask >= 0.5).to(torch.float32)


def keep_mask(mask):
    """bool [B, 1, H / 8, W / 8] from a mask [B, 1, H, W]"""
    return F.max_pool2d(binarise(mask), 8) < 0.5


def blend(latents, keep, z0, noise, k_x, k_n):
    """the select of the latent blend, in latents' dtype; (1, 0) stores z0 itself"""
    known = z0.double() if (k_x, k_n) == (1.0, 0.0) else k_x * z0.double() + k_n * noise.double()
    return torch.where(keep, known.to(latents.dtype), latents)


def sched_reference(sch, eps_seq, table, phi, lat0, keep, z0, noise, generator=None, seen=None):
    """tests/guidance_ref.py sched_reference with the blend after every step (float64).  keep bool [B, 1, h, w]; seen (a list) receives the
    blended latents of every evaluation"""
    B = lat0.shape[0]
    x = lat0.double()
    extra = {} if generator is None else {"generator": generator}
    assert len(table) == len(sch.timesteps) == eps_seq.shape[0]
    kc = keep_coeffs(sch)
    for i, t in enumerate(sch.timesteps):
        ec = eps_seq[i, B:].double()
        e = G.guided_eps(eps_seq[i, :B].double(), ec, table[i], phi) if G.is_cfg(table[i]) else ec
        x = sch.step(e, t, x, **extra).prev_sample
        x = blend(x, keep, z0, noise, *kc[i])
        if seen is not None:
            seen.append(x.clone())
    return x


def feather_weights(sigma):
    """float64 [2 r + 1], r = ceil(3 sigma), normalised"""
    r = int(math.ceil(3.0 * sigma))
    k = torch.arange(-r, r + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * k * k / (sigma * sigma))
    return w / w.sum(), r


def feather(mask_bin, sigma):
    """float64 separable Gaussian blur of a binarised mask [B, 1, H, W], replicate border"""
    w, r = feather_weights(sigma)
    m = F.conv2d(F.pad(mask_bin.double(), (r, r, 0, 0), mode="replicate"), w.view(1, 1, 1, -1))
    return F.conv2d(F.pad(m, (0, 0, r, r), mode="replicate"), w.view(1, 1, -1, 1))


def post(x):
    """clamp(x / 2 + 0.5, 0, 1) in float64"""
    return (x.double() / 2 + 0.5).clamp(0, 1)


def composite(decoded, image, m):
    """float64 [B, H, W, 3] from decoded / image [B, 3, H, W] (values in [-1, 1] before post) and m [B, 1, H, W]"""
    g, p, m = post(decoded), post(image), m.double()
    out = torch.where(m == 0, p, torch.where(m == 1, g, m * g + (1 - m) * p))
    return out.permute(0, 2, 3, 1)
