"""FreeU without a GPU: the closed form the kernel computes against diffusers' torch.fft formulation, the reference forward against the
oracle's (off: the same bits; on: every one of the four parameters is visible at the parity threshold the GPU tests use), the C surface and
the pipeline's argument check."""
from types import SimpleNamespace

import pytest
import torch

from oracle import configs as C
from oracle import models as M
from tests import freeu_ref as R
from tests import ref_unet as RU
from tests import util as U

FREEU = (0.9, 0.2, 1.4, 1.6)          # diffusers' recommendation for SD 2.1: s1, s2, b1, b2


@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (4, 3), (5, 3), (7, 5), (8, 6), (16, 12)])
@pytest.mark.parametrize("scale", [0.9, 0.2])
def test_closed_form_is_the_fft_filter(hw, scale):
    """fourier_filter_direct (at most four frequencies per plane, no FFT) against fftn -> fftshift -> box -> ifftshift -> ifftn in float64 on
    inputs of mean 3: <= 1e-12.  Size 2 has the Nyquist frequency as its -1, size 1 a single frequency"""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn((2, 3) + hw, generator=g, dtype=torch.float64) + 3.0
    ref = R.fourier_filter(x, 1, scale)
    got = R.fourier_filter_direct(x, scale)
    err = float((got - ref).abs().max())
    print("%dx%d scale %.1f: max |direct - fft| = %.3g" % (hw + (scale, err)))
    assert got.shape == ref.shape and err <= 1e-12, err
    if hw == (1, 1):
        assert torch.allclose(got, scale * x, rtol=0, atol=1e-12)         # the only frequency is in the box


@pytest.fixture(scope="module")
def tiny():
    torch.set_num_threads(U.cpu_quota_threads())
    cfg = C.UNET_TINY
    sd = C.synth_state_dict(C.unet_shapes(cfg), "unet.")
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 31, 32, 24), generator=g).half().float()
    ehs = torch.randn((2, 8, cfg["cross_attention_dim"]), generator=g).half().float()
    run = lambda fu: RU.unet_forward(sd, cfg, x, 481, ehs, freeu=fu)
    return dict(cfg=cfg, sd=sd, x=x, ehs=ehs, run=run, plain=M.unet_forward(sd, cfg, x, 481, ehs), on=run(FREEU))


def test_reference_off_is_the_oracle_forward(tiny):
    assert torch.equal(tiny["run"](None), tiny["plain"])


def test_every_parameter_is_visible_at_the_parity_threshold(tiny):
    """PSNR < 55 dB (the threshold of the GPU forward tests) between the FreeU forward and the plain one, and between the FreeU forward and
    the one with any single parameter at its neutral value 1 -- a library that dropped or swapped a parameter cannot pass those tests"""
    p = U.psnr(tiny["on"], tiny["plain"])
    print("FreeU %s against plain: %.1f dB" % (FREEU, p))
    assert p < 55.0, p
    arms = {"b only": (1.0, 1.0) + FREEU[2:], "s only": FREEU[:2] + (1.0, 1.0)}
    for i, name in enumerate(("s1", "s2", "b1", "b2")):
        arms["%s = 1" % name] = FREEU[:i] + (1.0,) + FREEU[i + 1:]
    arms["s2 = 0.5"] = (0.9, 0.5, 1.4, 1.6)
    for name, fu in arms.items():
        out = tiny["run"](fu)
        p_plain, p_on = U.psnr(out, tiny["plain"]), U.psnr(out, tiny["on"])
        print("%s: %.1f dB against plain, %.1f dB against %s" % (name, p_plain, p_on, FREEU))
        assert p_plain < 55.0 and p_on < 55.0, (name, p_plain, p_on)


def test_c_surface():
    """the library exports the setter and the operator; a null handle is refused with a message"""
    from ladi_vton_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "ladi_unet_set_freeu") and hasattr(lib, "ladi_op_freeu")
    assert lib.ladi_unet_set_freeu(None, 1, *FREEU) == -1
    assert "ladi_unet_set_freeu" in _lib.last_error()
    assert lib.ladi_unet_set_freeu(None, 0, 1.0, 1.0, 1.0, 1.0) == -1 and _lib.last_error()


def test_pipeline_needs_a_unet_with_freeu():
    import ladi_vton_amd as L

    class PlainUNet:
        config = SimpleNamespace(sample_size=8)

    pipe = L.StableDiffusionTryOnePipeline(vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=[1, 2, 3, 4])), text_encoder=None,
                                           tokenizer=None, unet=PlainUNet(), scheduler=L.DDIMScheduler())
    with pytest.raises(ValueError, match="PlainUNet"):
        pipe.enable_freeu(*FREEU)
    with pytest.raises(ValueError, match="PlainUNet"):
        pipe.disable_freeu()
    calls = []
    pipe.unet = SimpleNamespace(enable_freeu=lambda *a: calls.append(a), disable_freeu=lambda: calls.append(None))
    pipe.enable_freeu(*FREEU)
    pipe.disable_freeu()
    assert calls == [FREEU, None]
