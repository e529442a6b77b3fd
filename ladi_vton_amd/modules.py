"""Drop-in module shims over libladi_native: the nn.Module duck types StableDiffusionTryOnePipeline is built from
(reference: src/vto_pipelines/tryon_pipe.py:56-68,129-137; src/inference.py:212-220).

Each class exposes exactly the attributes / call conventions the reference pipeline touches and forwards the arithmetic to the
C ABI.  Tensors crossing between our own modules (the encoder features / EMASC skips) are NCHW-shaped views of NHWC fp16
buffers (channels_last strides), so no layout conversion happens between them.
"""
import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import (AdapterConfig, EMASCConfig, NativeError, UNetConfig, VAEConfig, check, dtype_code, ptr, stream_ptr)


# ---------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------
class _Weights:
    """host staging of a diffusers-format state_dict (ladi_weights_*)"""

    def __init__(self, state_dict):
        self.lib = _lib.load()
        self.h = self.lib.ladi_weights_create()
        if not self.h:
            raise NativeError("ladi_weights_create failed")
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict   # dict or iterator of (key, tensor) pairs
        for k, v in items:
            t = v.detach().to("cpu")
            if t.dtype not in (torch.float32, torch.float16):
                t = t.float()
            t = t.contiguous()
            shape = (c_int64 * max(t.dim(), 1))(*t.shape)
            check(self.lib.ladi_weights_add(self.h, k.encode(), c_void_p(t.data_ptr()), dtype_code(t), t.dim(), shape), "ladi_weights_add(%s)" % k)

    def close(self):
        if self.h:
            self.lib.ladi_weights_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _is_nhwc_dense(t):
    return t.dim() == 4 and t.dtype == torch.float16 and t.permute(0, 2, 3, 1).is_contiguous()


def _nhwc_buffer(t):
    """return an NHWC-dense fp16 [B,H,W,C] tensor holding `t` ([B,C,H,W] any strides / fp32|fp16) using the native converter"""
    if _is_nhwc_dense(t):
        return t.permute(0, 2, 3, 1)
    lib = _lib.load()
    src = t.contiguous()
    B, C, H, W = src.shape
    out = torch.empty((B, H, W, C), dtype=torch.float16, device=src.device)
    check(lib.ladi_op_nchw_to_nhwc(ptr(src), dtype_code(src), B, C, H, W, ptr(out), C, stream_ptr()), "nchw_to_nhwc")
    return out


class _Shim:
    """the nn.Module housekeeping the unmodified src/inference.py:192-209 performs on every module (`.to(device, dtype=...)`, `.eval()`):
    no-ops here, the weights already live on the device in the native layout"""

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def half(self):
        return self

    def float(self):
        return self

    def requires_grad_(self, requires_grad=False):
        return self

    def modules(self):
        return iter(())

    def parameters(self):
        return iter(())


class _Base(_Shim):
    dtype = torch.float16

    @property
    def device(self):
        return torch.device("cuda", torch.cuda.current_device())


# ---------------------------------------------------------------------------------------------------------------
# UNet (tryon_pipe.py:732: unet(x, t, encoder_hidden_states=...).sample)
# ---------------------------------------------------------------------------------------------------------------
class NativeUNet(_Base):
    def __init__(self, cfg, state_dict):
        _lib.require_gpu()
        self.lib = _lib.load()
        c = UNetConfig()
        c.in_channels, c.out_channels = cfg["in_channels"], cfg["out_channels"]
        c.block_out_channels = (c_int * 4)(*cfg["block_out_channels"])
        c.num_heads = (c_int * 4)(*cfg["num_heads"])
        c.layers_per_block, c.cross_attention_dim = cfg["layers_per_block"], cfg["cross_attention_dim"]
        c.norm_num_groups, c.norm_eps = cfg["norm_num_groups"], cfg["norm_eps"]
        with _Weights(state_dict) as w:
            self.h = self.lib.ladi_unet_create(ctypes.byref(c), w.h)
        if not self.h:
            raise NativeError("ladi_unet_create failed: " + _lib.last_error())
        self.cfg = dict(cfg)
        self.config = SimpleNamespace(in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], sample_size=64,
                                      _diffusers_version="0.14.0")
        self._ctx_key = None
        self._ctx_keepalive = None
        self.freeu = None             # (s1, s2, b1, b2) while FreeU is on
        self._lora_disabled = None    # the active set disable_lora() put aside for enable_lora()
        self._ip_key = None           # the image context the library holds (the tensor is kept alive, as for _ctx_key)
        self._ip_keepalive = None
        self._sag_last = None         # (samples of the context batch, h, w) of the last forward, for sag_map()'s defaults

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ladi_unet_destroy(self.h)
            self.h = None

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' UNet2DConditionModel.enable_freeu: in up_blocks.0 (s1, b1) and up_blocks.1 (s2, b2) the first half of the backbone
        channels is scaled by b and the skip's lowest frequencies by s before each concatenation.  Holds for every later forward of this
        UNet, stand-alone or inside the fused loop, until disable_freeu()."""
        v = tuple(float(x) for x in (s1, s2, b1, b2))
        check(self.lib.ladi_unet_set_freeu(self.h, 1, *v), "ladi_unet_set_freeu")
        self.freeu = v

    def disable_freeu(self):
        check(self.lib.ladi_unet_set_freeu(self.h, 0, 1.0, 1.0, 1.0, 1.0), "ladi_unet_set_freeu")
        self.freeu = None

    def set_pag_applied_layers(self, layers):
        """diffusers' pag_applied_layers: the transformer blocks in which a perturbed sample's self-attention map is the identity
        ("mid", "down", "up", "down.block_1", "up.block_2.attentions_0", .. as one string or a list; pipeline.pag_layer_mask), or the bit
        mask itself.  Sticky; the default is "mid".  It has no effect on a forward without perturbed samples (pag_first)."""
        if isinstance(layers, bool) or not isinstance(layers, int):
            from .pipeline import pag_layer_mask
            layers = pag_layer_mask(layers, self.cfg["layers_per_block"])
        if layers < 0 or layers >> 32:
            raise ValueError("the PAG layer mask has to fit 32 bits but is %r" % (layers,))
        check(self.lib.ladi_unet_set_pag_layers(self.h, layers), "ladi_unet_set_pag_layers")

    @property
    def pag_applied_layers(self):
        """the mask of selected transformer blocks, bit i = block i in execution order"""
        return int(self.lib.ladi_unet_pag_layers(self.h))

    # ---- self-attention guidance (include/ladi_native.h "Self-attention guidance"): the mid block's attention column sums
    def set_sag_capture(self, on):
        """Sticky, off by default.  On: every forward of this UNet also leaves the SAG map of mid_block.attentions.0's self-attention
        (sag_map()); the forward's output does not change.  A fused run with sag_scale > 0 captures whatever this says."""
        check(self.lib.ladi_unet_set_sag_capture(self.h, 1 if on else 0), "ladi_unet_set_sag_capture")

    def sag_tokens(self, h, w):
        """-> (hm, wm), the mid block's map size for h x w latents"""
        hm, wm = c_int(0), c_int(0)
        check(self.lib.ladi_unet_sag_tokens(self.h, int(h), int(w), ctypes.byref(hm), ctypes.byref(wm)), "ladi_unet_sag_tokens")
        return hm.value, wm.value

    def sag_map(self, n=None, latent_size=None):
        """-> (s, m) of the last capturing forward: s fp32 [n, hm, wm], the column sums sum_i mean_h softmax(q k^T / 8)[i, j] of the mid block's
        self-attention, and m uint8 [n, hm, wm] = s > 1, for the first n samples of the encoder_hidden_states batch.  n and latent_size
        (h, w) default to the last forward's through this object."""
        if n is None or latent_size is None:
            if self._sag_last is None:
                raise ValueError("sag_map() needs n and latent_size=(h, w): no forward has run through this object")
            n = self._sag_last[0] if n is None else n
            latent_size = self._sag_last[1:] if latent_size is None else latent_size
        hm, wm = self.sag_tokens(*latent_size)
        dev = torch.device("cuda", torch.cuda.current_device())
        s = torch.empty((int(n), hm, wm), dtype=torch.float32, device=dev)
        m = torch.empty((int(n), hm, wm), dtype=torch.uint8, device=dev)
        check(self.lib.ladi_unet_sag_map(self.h, ptr(s), ptr(m), int(n), hm * wm), "ladi_unet_sag_map")
        return s, m

    # ---- LoRA (lora.py, include/ladi_native.h "LoRA adapters"): merged onto the device weights, which keep their addresses
    def lora_target_modules(self):
        """the diffusers names of the modules a LoRA factor pair may be attached to: every conv and linear of this UNet"""
        from . import lora
        return lora.target_modules(self.cfg)

    def load_lora_adapter(self, state_dict, adapter_name="default"):
        """Load a LoRA state dict (PEFT, legacy diffusers or kohya keys: lora.normalize_state_dict) under adapter_name.  Everything is checked
        before anything changes.  Loading does not activate: set_adapters does.  Returns the keys that belong to a text encoder (not applied)."""
        from . import lora
        norm = lora.normalize_state_dict(state_dict, self.lora_target_modules())
        with _Weights(lora.to_library_keys(norm)) as w:
            check(self.lib.ladi_unet_lora_load(self.h, str(adapter_name).encode(), w.h), "ladi_unet_lora_load")
        return list(norm.text_encoder_keys)

    def set_adapters(self, names, weights=None):
        """diffusers' set_adapters: the active adapters, merged in this order at these weights (default 1.0 each); [] restores the plain
        weights bit for bit.  Every touched weight is re-merged from its pristine copy (no drift), on the device.  Raises, with the previous
        set back in place, when a merged weight leaves the fp16 range."""
        names = [names] if isinstance(names, str) else list(names)
        if weights is None:
            weights = [1.0] * len(names)
        elif isinstance(weights, (int, float)):
            weights = [float(weights)] * len(names)
        weights = [float(x) for x in weights]
        if len(weights) != len(names):
            raise ValueError("%d adapter names but %d weights" % (len(names), len(weights)))
        n = len(names)
        na = (ctypes.c_char_p * max(n, 1))(*[str(s).encode() for s in names])
        wa = (c_float * max(n, 1))(*weights)
        self._ctx_key = None           # whatever happens next, the cross-attention K/V cache no longer belongs to these weights
        check(self.lib.ladi_unet_set_adapters(self.h, na, wa, n, stream_ptr()), "ladi_unet_set_adapters")
        self._lora_disabled = None

    def disable_lora(self):
        """the plain weights, bit for bit; enable_lora() brings the set that was active back"""
        saved = self.active_adapters
        self.set_adapters([])
        self._lora_disabled = saved

    def enable_lora(self):
        if self._lora_disabled:
            saved = self._lora_disabled
            self.set_adapters([s[0] for s in saved], [s[1] for s in saved])

    def delete_adapters(self, names):
        """free adapters; refused for one that is active"""
        for s in ([names] if isinstance(names, str) else list(names)):
            check(self.lib.ladi_unet_lora_delete(self.h, str(s).encode()), "ladi_unet_lora_delete")
            if self._lora_disabled:
                self._lora_disabled = [a for a in self._lora_disabled if a[0] != s] or None
        self._ctx_key = None

    @property
    def active_adapters(self):
        """[(name, weight), ..] in merge order"""
        na, wa = (ctypes.c_char_p * 8)(), (c_float * 8)()
        n = self.lib.ladi_unet_lora_active(self.h, na, wa, 8)
        if n < 0:
            raise NativeError("ladi_unet_lora_active failed: " + _lib.last_error())
        return [(na[i].decode(), float(wa[i])) for i in range(n)]

    def list_adapters(self):
        """the names of the loaded adapters, in load order"""
        n = self.lib.ladi_unet_lora_count(self.h)
        return [self.lib.ladi_unet_lora_name(self.h, i).decode() for i in range(n)]

    def export_weight(self, key):
        """the live value of a diffusers `.weight` key of a conv / linear, in diffusers shape (float32 holding fp16 values)"""
        n = self.lib.ladi_unet_export_weight(self.h, key.encode(), None, 0)
        if n < 0:
            raise NativeError("ladi_unet_export_weight(%s) failed: %s" % (key, _lib.last_error()))
        out = torch.empty(n, dtype=torch.float32)
        if self.lib.ladi_unet_export_weight(self.h, key.encode(), c_void_p(out.data_ptr()), n) != n:
            raise NativeError("ladi_unet_export_weight(%s) failed: %s" % (key, _lib.last_error()))
        from . import configs
        return out.reshape(configs.unet_shapes(self.cfg)[key])

    def export_state_dict(self, base=None):
        """the live `.weight` of every conv and linear (the merged weights while adapters are active: a fused checkpoint).  base: a state dict
        whose other entries (norms, biases), which LoRA never touches, are carried over so that the result is a whole checkpoint"""
        from collections import OrderedDict
        out = OrderedDict((k, v) for k, v in base.items()) if base is not None else OrderedDict()
        for m in self.lora_target_modules():
            out[m + ".weight"] = self.export_weight(m + ".weight")
        return out

    # ---- IP-Adapter image prompt (ip_adapter.py, include/ladi_native.h "IP-Adapter image prompt")
    def load_ip_adapter(self, state_dict_or_path, image_proj_dim_head=64):
        """Load an IP-Adapter (diffusers' {"image_proj", "ip_adapter"} layout, nested or flat, numbered or module-named keys:
        ip_adapter.load_state).  Everything is checked before anything changes; one adapter per UNet.  Loading activates nothing: an image
        term appears in a forward that is given ip_image_embeds= / ip_tokens=.  A new adapter starts with every scale 1.0.
        A Plus checkpoint (image_proj is a Resampler) is loaded with its Resampler, built with heads of image_proj_dim_head (the weights
        do not record it; 64 in the released files); ip_image_embeds= then takes hidden states [n, T, E]."""
        from . import ip_adapter
        sd = ip_adapter.load_state(state_dict_or_path, self.cfg["layers_per_block"])
        with _Weights(sd) as w:
            check(self.lib.ladi_unet_ip_adapter_load_ex(self.h, w.h, int(image_proj_dim_head)), "ladi_unet_ip_adapter_load_ex")
        self._ip_key = self._ip_keepalive = None

    def unload_ip_adapter(self):
        check(self.lib.ladi_unet_ip_adapter_unload(self.h), "ladi_unet_ip_adapter_unload")
        self._ip_key = self._ip_keepalive = None

    @property
    def ip_adapter_info(self):
        """None, or (tokens per image, embedding width) of the loaded adapter"""
        n, e = c_int(0), c_int(0)
        rc = self.lib.ladi_unet_ip_adapter_info(self.h, ctypes.byref(n), ctypes.byref(e))
        if rc < 0:
            raise NativeError("ladi_unet_ip_adapter_info failed: " + _lib.last_error())
        return (n.value, e.value) if rc else None

    @property
    def ip_adapter_is_plus(self):
        """True when the loaded adapter's image projection is a Resampler (it reads hidden states [n, T, E], not one embedding per image)"""
        rc = self.lib.ladi_unet_ip_adapter_is_plus(self.h)
        if rc < 0:
            raise NativeError("ladi_unet_ip_adapter_is_plus failed: " + _lib.last_error())
        return bool(rc)

    def set_ip_adapter_scale(self, scale):
        """diffusers' set_ip_adapter_scale: a number (every transformer block), or a dict / list of (name, scale) in the block names of
        set_pag_applied_layers ("down", "up.block_1", "mid", ..), unnamed blocks 0 -- the layer-wise use of diffusers' dict form.  Sticky; a
        block with scale 0 launches nothing for the image term."""
        from . import ip_adapter
        v = ip_adapter.scale_list(scale, self.cfg["layers_per_block"])
        check(self.lib.ladi_unet_set_ip_scale(self.h, (c_float * len(v))(*v), len(v)), "ladi_unet_set_ip_scale")

    @property
    def ip_adapter_scale(self):
        """the scale of every transformer block, in execution order"""
        out = (c_float * 32)()
        n = self.lib.ladi_unet_ip_scale(self.h, out, 32)
        if n < 0:
            raise NativeError("ladi_unet_ip_scale failed: " + _lib.last_error())
        return [float(out[i]) for i in range(n)]

    def set_ip_context(self, embeds=None, tokens=None):
        """the image context of the following forwards: embeds [n, E] (or [n, 1, E]) through the adapter's projection -- with a Plus adapter
        hidden states [n, T, E] through its Resampler (ladi_unet_set_ip_context_seq) --, or finished tokens [n, N, cross_dim]; both None:
        none.  The same tensor object passed again unmodified is not uploaded again."""
        if embeds is not None and tokens is not None:
            raise ValueError("`ip_image_embeds` and `ip_tokens` cannot both be given.")
        t = embeds if embeds is not None else tokens
        if t is None:
            if self._ip_key != "none":
                check(self.lib.ladi_unet_clear_ip_context(self.h), "ladi_unet_clear_ip_context")
                self._ip_key, self._ip_keepalive = "none", None
            return
        info = self.ip_adapter_info
        if info is None:
            raise ValueError("an image prompt needs a loaded IP-Adapter (load_ip_adapter).")
        key = (id(t), t._version, embeds is not None)
        if self._ip_key == key and self._ip_keepalive is not None and self._ip_keepalive[0] is t:
            return
        if embeds is not None and self.ip_adapter_is_plus:
            if embeds.dim() != 3 or embeds.shape[1] < 1 or embeds.shape[2] != info[1]:
                raise ValueError("ip_image_embeds has shape %s, but the loaded adapter is a Plus adapter: expected hidden states [n, T, %d] "
                                 "(the image encoder's hidden_states[-2])" % (tuple(embeds.shape), info[1]))
            e = embeds.to(device=self.device, dtype=torch.float16).contiguous()
            check(self.lib.ladi_unet_set_ip_context_seq(self.h, ptr(e), e.shape[0], e.shape[1], stream_ptr()), "ladi_unet_set_ip_context_seq")
        elif embeds is not None:
            e = embeds[:, 0] if embeds.dim() == 3 and embeds.shape[1] == 1 else embeds
            if e.dim() != 2 or e.shape[1] != info[1]:
                raise ValueError("ip_image_embeds has shape %s, expected [n, %d] (the loaded adapter's embedding width)" % (tuple(embeds.shape), info[1]))
            e = e.to(device=self.device, dtype=torch.float16).contiguous()
            check(self.lib.ladi_unet_set_ip_context(self.h, ptr(e), e.shape[0], stream_ptr()), "ladi_unet_set_ip_context")
        else:
            if tokens.dim() != 3 or tokens.shape[2] != self.cfg["cross_attention_dim"] or not 1 <= tokens.shape[1] <= 64:
                raise ValueError("ip_tokens has shape %s, expected [n, N <= 64, %d]" % (tuple(tokens.shape), self.cfg["cross_attention_dim"]))
            e = tokens.to(device=self.device, dtype=torch.float16).contiguous()
            check(self.lib.ladi_unet_set_ip_tokens(self.h, ptr(e), e.shape[0], e.shape[1], stream_ptr()), "ladi_unet_set_ip_tokens")
        self._ip_key, self._ip_keepalive = key, (t, e)

    # ---- token merging (tome.py, include/ladi_native.h "Token merging")
    def set_token_merging(self, ratio=0.5, **kw):
        """tomesd.apply_patch for this UNet: the transformer blocks of the first max_downsample levels run the selected sub-layers over
        T - int(T * ratio) rows (tome.config's keywords: max_downsample, sx, sy, use_rand, seed, merge_attn, merge_crossattn, merge_mlp).
        ratio None or 0: off, the plain forward launch for launch.  Sticky, for every later forward, stand-alone or in the fused loop."""
        from . import tome
        if ratio is None:
            check(self.lib.ladi_unet_set_token_merging(self.h, None), "ladi_unet_set_token_merging")
            return
        cfg = tome.config(ratio, **kw)
        c = _lib.ToMeConfig(**{k: (int(v) if isinstance(v, bool) else v) for k, v in cfg.items()})
        check(self.lib.ladi_unet_set_token_merging(self.h, ctypes.byref(c)), "ladi_unet_set_token_merging")

    def remove_token_merging(self):
        self.set_token_merging(None)

    @property
    def token_merging(self):
        """None while off, else the configuration as a dict"""
        c = _lib.ToMeConfig()
        rc = self.lib.ladi_unet_token_merging(self.h, ctypes.byref(c))
        if rc < 0:
            raise NativeError("ladi_unet_token_merging failed: " + _lib.last_error())
        if not rc:
            return None
        return dict(ratio=c.ratio, max_downsample=c.max_downsample, sx=c.sx, sy=c.sy, use_rand=bool(c.use_rand), seed=int(c.seed),
                    merge_attn=bool(c.merge_attn), merge_crossattn=bool(c.merge_crossattn), merge_mlp=bool(c.merge_mlp))

    def token_merging_blocks(self):
        """the merged transformer blocks, as indices in execution order (the numbering of the PAG layer mask)"""
        out = (c_int * 32)()
        n = self.lib.ladi_unet_tome_block_count(self.h, out, 32)
        if n < 0:
            raise NativeError("ladi_unet_tome_block_count failed: " + _lib.last_error())
        return [int(out[i]) for i in range(n)]

    def token_merging_plan(self, block):
        """out_row of the block-th merged block as the last forward left it: a flat int32 tensor of n * T entries, entry s * T + p the row of the
        merged sequence token p of sample s reads (tokens that share a value were merged); None when the block merged nothing"""
        n = self.lib.ladi_unet_tome_read_plan(self.h, int(block), None, 0)
        if n < 0:
            raise NativeError("ladi_unet_tome_read_plan failed: " + _lib.last_error())
        if n == 0:
            return None
        out = torch.empty(n, dtype=torch.int32)
        if self.lib.ladi_unet_tome_read_plan(self.h, int(block), c_void_p(out.data_ptr()), n) != n:
            raise NativeError("ladi_unet_tome_read_plan failed: " + _lib.last_error())
        return out

    def enable_xformers_memory_efficient_attention(self, *a, **k):
        return None  # attention is always fused (flash-style) in the native kernels

    def set_context(self, ehs):
        # the cross-attention K/V projections are step-invariant: skip the upload when the SAME tensor object (kept alive here, so its
        # id / storage cannot be recycled by the caching allocator) is passed again unmodified
        key = (id(ehs), ehs._version)
        if self._ctx_key == key and self._ctx_keepalive is not None and self._ctx_keepalive[0] is ehs:
            return
        e = ehs.to(dtype=torch.float16).contiguous()
        check(self.lib.ladi_unet_set_context(self.h, ptr(e), e.shape[0], e.shape[1], stream_ptr()), "ladi_unet_set_context")
        self._ctx_key = key
        self._ctx_keepalive = (ehs, e)

    FEATURE_CACHE_MODES = {None: 0, "capture": 1, "reuse": 2}

    def __call__(self, sample, timestep, encoder_hidden_states=None, feature_cache=None, cache_branch=0, sample0=0, pag_first=None,
                 ip_image_embeds=None, ip_tokens=None, **kw):
        """ip_image_embeds / ip_tokens: the image prompt of this forward (set_ip_context), one row per sample of the
        encoder_hidden_states batch; neither: no image term, the plain forward.
        pag_first: None, or the index in the encoder_hidden_states batch from which the samples are perturbed (perturbed-attention
        guidance: identity self-attention in the blocks of set_pag_applied_layers); not together with feature_cache.
        feature_cache: None, "capture" (the whole forward, which also caches the deep features of the full-resolution level) or "reuse"
        (the shallow forward from that cache: the outermost cache_branch + 1 layers only; ladi_unet_forward_cached).  sample0: the samples
        are rows [sample0, sample0 + n) of the encoder_hidden_states batch (their own rows of the K/V and feature caches)."""
        if encoder_hidden_states is None:
            raise ValueError("encoder_hidden_states is required")
        if feature_cache not in self.FEATURE_CACHE_MODES:
            raise ValueError("feature_cache has to be None, 'capture' or 'reuse' but is %r" % (feature_cache,))
        if isinstance(cache_branch, bool) or not isinstance(cache_branch, int) or not 0 <= cache_branch <= self.cfg["layers_per_block"]:
            raise ValueError("cache_branch has to be in [0, %d] but is %r" % (self.cfg["layers_per_block"], cache_branch))
        self.set_context(encoder_hidden_states)
        self.set_ip_context(ip_image_embeds, ip_tokens)
        x = sample.contiguous()
        n, C, h, w = x.shape
        if C != self.cfg["in_channels"]:
            raise ValueError("expected %d input channels, got %d" % (self.cfg["in_channels"], C))
        out = torch.empty((n, self.cfg["out_channels"], h, w), dtype=x.dtype, device=x.device)
        self._sag_last = (int(sample0) + n, h, w)
        if pag_first is not None:
            if feature_cache is not None:
                raise ValueError("`pag_first` and `feature_cache` cannot be combined.")
            if isinstance(pag_first, bool) or not isinstance(pag_first, int) or pag_first < 0:
                raise ValueError("pag_first has to be a non-negative int but is %r" % (pag_first,))
            check(self.lib.ladi_unet_forward_pag(self.h, ptr(x), dtype_code(x), n, h, w, float(timestep), ptr(out), dtype_code(out), int(sample0),
                                                 pag_first, stream_ptr()), "ladi_unet_forward_pag")
            return SimpleNamespace(sample=out)
        if feature_cache is not None or sample0:
            check(self.lib.ladi_unet_forward_cached_rows(self.h, ptr(x), dtype_code(x), n, h, w, float(timestep), ptr(out), dtype_code(out),
                                                         self.FEATURE_CACHE_MODES[feature_cache], int(cache_branch), int(sample0), stream_ptr()),
                  "ladi_unet_forward_cached")
            return SimpleNamespace(sample=out)
        check(self.lib.ladi_unet_forward(self.h, ptr(x), dtype_code(x), n, h, w, float(timestep), ptr(out), dtype_code(out), stream_ptr()),
              "ladi_unet_forward")
        return SimpleNamespace(sample=out)

    def time_forward(self, n, h, w, iters):
        ms = c_float(0)
        check(self.lib.ladi_unet_time_forward(self.h, n, h, w, iters, ctypes.byref(ms), stream_ptr()), "ladi_unet_time_forward")
        return ms.value

    def time_forward_cached(self, n, h, w, iters, feature_cache="reuse", cache_branch=0):
        """average ms of one forward in a feature-cache mode ("capture" / "reuse"), measured like time_forward"""
        ms = c_float(0)
        check(self.lib.ladi_unet_time_forward_cached(self.h, n, h, w, iters, self.FEATURE_CACHE_MODES[feature_cache], int(cache_branch),
                                                     ctypes.byref(ms), stream_ptr()), "ladi_unet_time_forward_cached")
        return ms.value

    def time_forward_lanes(self, n, h, w, iters, lanes=0, use_graph=True):
        """average ms of one forward run the way the denoising loop runs it: `lanes` sample groups on as many streams, one hipGraph"""
        ms = c_float(0)
        check(self.lib.ladi_unet_time_forward_lanes(self.h, n, h, w, iters, lanes, 1 if use_graph else 0, ctypes.byref(ms), stream_ptr()),
              "ladi_unet_time_forward_lanes")
        return ms.value


# ---------------------------------------------------------------------------------------------------------------
# VAE (AutoencoderKL.encode / .decode with EMASC wiring)
# ---------------------------------------------------------------------------------------------------------------
class DiagonalGaussianDistribution:
    """src/models/vae.py:329-348 over moments produced natively"""

    def __init__(self, parameters):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator=None, noise=None):
        if noise is None:
            dev = generator.device if generator is not None else self.mean.device
            noise = torch.randn(self.mean.shape, generator=generator, device=dev, dtype=self.mean.dtype).to(self.mean.device)
        return self.mean + self.std * noise.to(self.mean.dtype)

    def mode(self):
        return self.mean


class NativeVAE(_Base):
    def __init__(self, cfg, state_dict):
        _lib.require_gpu()
        self.lib = _lib.load()
        c = VAEConfig()
        c.in_channels, c.out_channels, c.latent_channels = cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"]
        c.block_out_channels = (c_int * 4)(*cfg["block_out_channels"])
        c.layers_per_block, c.norm_num_groups, c.scaling_factor = cfg["layers_per_block"], cfg["norm_num_groups"], cfg["scaling_factor"]
        with _Weights(state_dict) as w:
            self.h = self.lib.ladi_vae_create(ctypes.byref(c), w.h)
        if not self.h:
            raise NativeError("ladi_vae_create failed: " + _lib.last_error())
        self.cfg = dict(cfg)
        self.config = SimpleNamespace(scaling_factor=cfg["scaling_factor"], latent_channels=cfg["latent_channels"],
                                      block_out_channels=tuple(cfg["block_out_channels"]))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ladi_vae_destroy(self.h)
            self.h = None

    @property
    def range_shift(self):
        """fp16-range guard of the decoder: "auto" (default) decodes with the residual stream at its true scale and, when a GroupNorm
        reports non-finite statistics (an fp16 overflow upstream), again with the stream stored x 2^-4, then 2^-8; an int k fixes the stream
        scale at 2^-k.  The reference decodes in whatever dtype the caller chose (src/models/AutoencoderKL.py:159-188); SD VAE checkpoints
        are known to leave the fp16 range there.  `last_range_shift` tells what the last decode used."""
        return getattr(self, "_range_shift", "auto")

    @range_shift.setter
    def range_shift(self, k):
        kk = -1 if k in ("auto", None) else int(k)
        check(self.lib.ladi_vae_set_range_shift(self.h, kk), "ladi_vae_set_range_shift")
        self._range_shift = "auto" if kk < 0 else kk

    @property
    def last_range_shift(self):
        return self.lib.ladi_vae_last_range_shift(self.h)

    def encode(self, x, return_dict=True):
        x = x.contiguous()
        B, _, H, W = x.shape
        boc = self.cfg["block_out_channels"]
        dev = x.device
        moments = torch.empty((B, 2 * self.cfg["latent_channels"], H // 8, W // 8), dtype=torch.float32, device=dev)
        shapes = [(B, H, W, boc[0]), None, (B, H // 2, W // 2, boc[0]), (B, H // 4, W // 4, boc[1]), (B, H // 8, W // 8, boc[2])]
        bufs = [torch.empty(s, dtype=torch.float16, device=dev) if s else None for s in shapes]
        arr = (c_void_p * 5)(*[b.data_ptr() if b is not None else None for b in bufs])
        check(self.lib.ladi_vae_encode(self.h, ptr(x), dtype_code(x), B, H, W, ptr(moments), arr, stream_ptr()), "ladi_vae_encode")
        views = [b.permute(0, 3, 1, 2) if b is not None else None for b in bufs]
        views[1] = views[0]  # idx1 and idx2 are the same tensor in the reference (vae.py:104-109)
        feats = [x] + views
        post = DiagonalGaussianDistribution(moments.to(x.dtype) if x.dtype == torch.float16 else moments)
        if not return_dict:
            return (post,)
        return SimpleNamespace(latent_dist=post), feats

    def decode(self, z, intermediate_features=None, int_layers=None, return_dict=True):
        B, _, h, w = z.shape
        zf = z.float().contiguous()
        arr = None
        keep = []
        if intermediate_features:
            # Decoder.forward (vae.py:188-205) zips the REVERSED list with the four up blocks (a list shorter than four silently SKIPS the
            # remaining up blocks, which the released channel widths then reject at conv_norm_out) and adds layer 1 after conv_norm_out:
            # the only selections whose shapes line up are [1, 2, 3, 4, 5] and [2, 3, 4, 5]
            layers = list(int_layers or [])
            if layers not in ([1, 2, 3, 4, 5], [2, 3, 4, 5]) or len(intermediate_features) != len(layers):
                raise ValueError("int_layers must be [1, 2, 3, 4, 5] or [2, 3, 4, 5] with one feature per layer (got %r with %d features): "
                                 "the reference's Decoder.forward cannot run any other selection on the released architecture"
                                 % (int_layers, len(intermediate_features)))
            keep = [_nhwc_buffer(f) for f in intermediate_features]
            slots = [None] * 5
            for layer, k in zip(layers, keep):
                slots[layer - 1] = k.data_ptr()
            arr = (c_void_p * 5)(*slots)
            intermediate_features.reverse()  # the reference reverses the caller's list in place (vae.py:190)
        out = torch.empty((B, self.cfg["out_channels"], 8 * h, 8 * w), dtype=z.dtype if z.dtype in (torch.float16, torch.float32) else torch.float32,
                          device=z.device)
        check(self.lib.ladi_vae_decode(self.h, ptr(zf), B, h, w, arr, ptr(out), dtype_code(out), stream_ptr()), "ladi_vae_decode")
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)


# ---------------------------------------------------------------------------------------------------------------
# EMASC + mask_features
# ---------------------------------------------------------------------------------------------------------------
class NativeEMASC(_Base):
    def __init__(self, cfg, state_dict):
        _lib.require_gpu()
        self.lib = _lib.load()
        c = EMASCConfig()
        n = len(cfg["in_channels"])
        c.n = n
        c.in_channels = (c_int * 8)(*(list(cfg["in_channels"]) + [0] * (8 - n)))
        c.out_channels = (c_int * 8)(*(list(cfg["out_channels"]) + [0] * (8 - n)))
        with _Weights(state_dict) as w:
            self.h = self.lib.ladi_emasc_create(ctypes.byref(c), w.h)
        if not self.h:
            raise NativeError("ladi_emasc_create failed: " + _lib.last_error())
        self.cfg = dict(cfg)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ladi_emasc_destroy(self.h)
            self.h = None

    def __bool__(self):
        return True

    def __call__(self, x, mask=None):
        """x: list of feature tensors (replaced in place like emasc.py:37-40). mask (optional extension): binarised
        [B,1,H,W] mask fused as mask_features."""
        n = len(self.cfg["in_channels"])
        if len(x) != n:
            raise ValueError("EMASC expects %d features" % n)
        src = [_nhwc_buffer(f) for f in x]
        B = src[0].shape[0]
        outs = [torch.empty((B, s.shape[1], s.shape[2], co), dtype=torch.float16, device=s.device) for s, co in zip(src, self.cfg["out_channels"])]
        fa = (c_void_p * n)(*[s.data_ptr() for s in src])
        oa = (c_void_p * n)(*[o.data_ptr() for o in outs])
        hs = (c_int * n)(*[s.shape[1] for s in src])
        ws = (c_int * n)(*[s.shape[2] for s in src])
        mk, Hm, Wm = None, 0, 0
        if mask is not None:
            mk = (mask >= 0.5).to(torch.float16).contiguous()
            Hm, Wm = mk.shape[-2:]
        check(self.lib.ladi_emasc_forward(self.h, fa, hs, ws, B, ptr(mk), Hm, Wm, oa, stream_ptr()), "ladi_emasc_forward")
        for i in range(n):
            x[i] = outs[i].permute(0, 3, 1, 2)
        return x


def mask_features(features, mask):
    """Native counterpart of src/utils/data_utils.py:4-16 on NHWC-backed features (in place)."""
    lib = _lib.load()
    mk = mask.to(torch.float16).contiguous()
    Hm, Wm = mk.shape[-2:]
    for i, f in enumerate(features):
        buf = _nhwc_buffer(f)
        B, h, w, C = buf.shape
        check(lib.ladi_mask_features(ptr(buf), B, h, w, C, ptr(mk), Hm, Wm, stream_ptr()), "ladi_mask_features")
        features[i] = buf.permute(0, 3, 1, 2)
    return features


# ---------------------------------------------------------------------------------------------------------------
# inversion adapter (inference.py:276)
# ---------------------------------------------------------------------------------------------------------------
class NativeInversionAdapter(_Base):
    def __init__(self, cfg, state_dict):
        _lib.require_gpu()
        self.lib = _lib.load()
        c = AdapterConfig()
        c.hidden, c.heads, c.mlp_dim, c.head_hidden, c.out_dim = cfg["hidden"], cfg["heads"], cfg["mlp_dim"], cfg["head_hidden"], cfg["out_dim"]
        c.layer_norm_eps = cfg["layer_norm_eps"]
        with _Weights(state_dict) as w:
            self.h = self.lib.ladi_adapter_create(ctypes.byref(c), w.h)
        if not self.h:
            raise NativeError("ladi_adapter_create failed: " + _lib.last_error())
        self.cfg = dict(cfg)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ladi_adapter_destroy(self.h)
            self.h = None

    def __call__(self, x):
        xin = x.to(torch.float16).contiguous()
        B, T, H = xin.shape
        out = torch.empty((B, self.cfg["out_dim"]), dtype=torch.float16, device=xin.device)
        check(self.lib.ladi_adapter_forward(self.h, ptr(xin), B, T, ptr(out), stream_ptr()), "ladi_adapter_forward")
        return out.to(x.dtype) if x.dtype in (torch.float32,) else out
