"""The image projection of IP-Adapter Plus as a native module: the tencent-ailab `Resampler` (a Perceiver resampler) over libladi_native
(include/ladi_native.h "Resampler", csrc/runtime_resampler.cpp).

    resampler = NativeResampler(plus_checkpoint["image_proj"], dim_head=64)                  # once
    tokens = resampler(vision_encoder(pixel_values, output_hidden_states=True).hidden_states[-2])   # [n, T, E] -> [n, N, out_dim]

The arithmetic is restated from memory of the IP-Adapter package, which is not a dependency of this one, and was not checked against it:
N learned latents attend over [LayerNorm(proj_in(x)) ; LayerNorm(latents)] (T + N keys, logits / sqrt(dim_head), softmax in fp32) for
`depth` layers, each followed by a bias-free 4x GELU feed-forward, then proj_out and a LayerNorm; every LayerNorm with eps 1e-5.  The
state dict is the original key layout (latents, proj_in, proj_out, norm_out, layers.i.0.{norm1,norm2,to_q,to_kv,to_out},
layers.i.1.{0,1,3}); the geometry comes from the weights and heads = inner / dim_head.  No CPU fallback.
"""
import ctypes
from ctypes import c_int

import torch

from . import _lib
from ._lib import NativeError, check, ptr, stream_ptr
from .modules import _Base, _Weights


class NativeResampler(_Base):
    def __init__(self, state_dict, dim_head=64):
        self.lib = _lib.load()
        self.h = None
        with _Weights(state_dict) as w:
            self.h = self.lib.ladi_resampler_create(w.h, int(dim_head))
        if not self.h:
            raise NativeError("ladi_resampler_create failed: " + _lib.last_error())
        v = [c_int(0) for _ in range(6)]
        check(self.lib.ladi_resampler_info(self.h, *[ctypes.byref(x) for x in v]), "ladi_resampler_info")
        self.num_queries, self.embedding_dim, self.dim, self.depth, self.heads, self.output_dim = (x.value for x in v)
        self.dim_head = int(dim_head)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ladi_resampler_destroy(self.h)
            self.h = None

    def __call__(self, x, out=None):
        """x [n, T, E] -> tokens fp16 [n, N, out_dim] (written into `out` when given: fp16, contiguous, on the device)"""
        if x.dim() != 3 or x.shape[1] < 1 or x.shape[2] != self.embedding_dim:
            raise ValueError("the Resampler's input has shape %s, expected [n, T, %d]" % (tuple(x.shape), self.embedding_dim))
        x = x.to(device=self.device, dtype=torch.float16).contiguous()
        shape = (x.shape[0], self.num_queries, self.output_dim)
        if out is None:
            out = torch.empty(shape, dtype=torch.float16, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float16 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("`out` has to be a contiguous fp16 device tensor of shape %s" % (shape,))
        check(self.lib.ladi_resampler_forward(self.h, ptr(x), x.shape[0], x.shape[1], ptr(out), stream_ptr()), "ladi_resampler_forward")
        return out
