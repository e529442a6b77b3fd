"""Reference for FreeU (diffusers UNet2DConditionModel.enable_freeu): the yardstick tests/test_cpu_freeu.py and tests/test_gpu_freeu.py
compare the library with.  fourier_filter is diffusers' torch.fft formulation in float64, fourier_filter_direct the closed form the kernel
computes.  tests/ref_unet.py's forward calls apply_freeu before every concatenation of up_blocks.0 and up_blocks.1 (freeu=), tests/ref_tryon.py's
loop runs that forward.

    freeu                    None (off) or (s1, s2, b1, b2), diffusers' argument order: stage i uses s = freeu[i], b = freeu[2 + i]
    apply_freeu(i, h, sk)    i >= 2 or freeu None: unchanged; else h[:, :C // 2] * b and fourier_filter(sk, threshold = 1, scale = s)
"""
import math

import torch


def fourier_filter(x, threshold, scale):
    """diffusers.utils.torch_utils.fourier_filter on [B, C, H, W], in float64 -> float64"""
    x = x.double()
    B, C, H, W = x.shape
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = torch.fft.ifftshift(xf * mask, dim=(-2, -1))
    return torch.fft.ifftn(xf, dim=(-2, -1)).real


def low_pass(x):
    """the part of x [.., H, W] at the frequencies of fourier_filter's box for threshold 1: u in {0, -1 mod H}, v in {0, -1 mod W}, each
    distinct frequency once (an axis of length 1 has one, an axis of length 2 its mean and its Nyquist frequency); float64, no FFT"""
    x = x.double()
    H, W = x.shape[-2:]
    ys, xs = torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64)
    lp = torch.zeros_like(x)
    for u in sorted({0, (-1) % H}):
        for v in sorted({0, (-1) % W}):
            ey = torch.exp(-2j * math.pi * u * ys / H)
            ex = torch.exp(-2j * math.pi * v * xs / W)
            f = torch.einsum("...yx,y,x->...", x.to(torch.complex128), ey, ex)
            lp = lp + (f[..., None, None] * ey.conj()[:, None] * ex.conj()[None, :]).real
    return lp / (H * W)


def fourier_filter_direct(x, scale):
    """fourier_filter(x, 1, scale) in closed form: x + (scale - 1) low_pass(x)"""
    return x.double() + (scale - 1.0) * low_pass(x)


def apply_freeu(i, hidden, skip, freeu):
    """diffusers.utils.torch_utils.apply_freeu for up block i -> (hidden, skip), in the dtype they came in"""
    if freeu is None or i >= 2:
        return hidden, skip
    s, b = float(freeu[i]), float(freeu[2 + i])
    half = hidden.shape[1] // 2
    hidden = torch.cat([(hidden[:, :half].double() * b).to(hidden.dtype), hidden[:, half:]], dim=1)
    return hidden, fourier_filter(skip, 1, s).to(skip.dtype)
