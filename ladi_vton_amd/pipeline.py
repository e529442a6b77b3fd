"""StableDiffusionTryOnePipeline on the native modules — same constructor and __call__ signature as the reference
(src/vto_pipelines/tryon_pipe.py:56-68, 494-520), so src/inference.py:212-220,298-311 can use it unchanged.

Two execution modes with identical semantics:
  * fused (default): steps 4-11 run inside libladi_native (ladi_tryon_run), the denoising step hipGraph-captured;
  * modular (fused=False): the same stages driven from Python through the drop-in module shims, one C-ABI call per module.
"""
import ctypes
import inspect
import math
import numbers
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import TryOnInputs, check, dtype_code, ptr, stream_ptr
from .modules import NativeEMASC, NativeUNet, NativeVAE, mask_features
from .schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                         LCMScheduler, LMSDiscreteScheduler, PNDMScheduler, TCDScheduler)

# the schedulers the fused native loop runs (ladi_tryon_run): the native step table of each is the mirror's arithmetic
FUSED_SCHEDULERS = (DDIMScheduler, PNDMScheduler, LMSDiscreteScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
                    EulerAncestralDiscreteScheduler, LCMScheduler, TCDScheduler)


def guidance_interval(n_evals, scale, start=0.0, stop=1.0):
    """a guidance schedule for `guidance_scale=`: `scale` on the evaluations ceil(start * n_evals) <= i < ceil(stop * n_evals), 1.0 (cond-only:
    no unconditional forward) elsewhere"""
    n = int(n_evals)
    if n < 0 or not (0.0 <= start <= 1.0) or not (0.0 <= stop <= 1.0):
        raise ValueError("guidance_interval: n_evals >= 0 and start, stop in [0, 1]")
    lo, hi = math.ceil(start * n), math.ceil(stop * n)
    return [float(scale) if lo <= i < hi else 1.0 for i in range(n)]


def guidance_plan(guidance_scale, n_evals, guidance_rescale=0.0):
    """-> (table, scalar, do_cfg).  guidance_scale: a float (table is None: one scale for the run), a sequence of n_evals scales, or a
    callable f(i, n_evals); n_evals: len(scheduler.timesteps) or a callable returning it (only asked for a schedule).  do_cfg: any scale > 1.
    An evaluation whose scale is <= 1 runs cond-only.  Raises ValueError for a wrong length, a negative or non-finite entry, or a
    guidance_rescale outside [0, 1]."""
    phi = float(guidance_rescale)
    if not (0.0 <= phi <= 1.0):
        raise ValueError("`guidance_rescale` has to be in [0, 1] but is %r." % (guidance_rescale,))
    if isinstance(guidance_scale, numbers.Real) or (not callable(guidance_scale) and getattr(guidance_scale, "ndim", 1) == 0):
        return None, float(guidance_scale), float(guidance_scale) > 1.0
    n = int(n_evals() if callable(n_evals) else n_evals)
    if callable(guidance_scale):
        table = [float(guidance_scale(i, n)) for i in range(n)]
    else:
        table = [float(g) for g in guidance_scale]
        if len(table) != n:
            raise ValueError("`guidance_scale` has %d entries but the scheduler runs %d evaluations (len(scheduler.timesteps))." % (len(table), n))
    for i, g in enumerate(table):
        if not math.isfinite(g) or g < 0.0:
            raise ValueError("`guidance_scale[%d]` = %r: every scale has to be finite and >= 0." % (i, g))
    return table, (table[0] if table else 1.0), any(g > 1.0 for g in table)


def feature_cache_plan(n_evals, interval, cond_only=None):
    """-> one bool per evaluation, True = whole UNet forward (which refreshes the deep-feature cache), False = shallow forward from the cache,
    after the loop's one promotion.  interval: an int N >= 1 (whole at i % N == 0) or a sequence of n_evals truthy / falsy entries; entry 0 is
    always whole.  cond_only: None, or one truthy entry per evaluation that runs cond-only inside a CFG-shaped run (a guidance schedule's
    scale <= 1).  Promotion: a shallow evaluation over all 2B samples needs both halves of the cache from the same whole evaluation, so when
    the most recent whole evaluation ran cond-only it runs whole instead; a shallow cond-only evaluation is never promoted.  Raises ValueError
    for an interval < 1 or of another type, or a sequence of the wrong length."""
    n = int(n_evals)
    if n < 0:
        raise ValueError("feature_cache_plan: n_evals >= 0")
    if isinstance(interval, bool) or (isinstance(interval, numbers.Real) and not isinstance(interval, numbers.Integral)):
        raise ValueError("`feature_cache` interval has to be an integer >= 1 but is %r." % (interval,))
    if isinstance(interval, numbers.Integral):
        if interval < 1:
            raise ValueError("`feature_cache` interval has to be an integer >= 1 but is %r." % (interval,))
        flags = [i % int(interval) == 0 for i in range(n)]
    else:
        try:
            flags = [bool(f) for f in interval]
        except TypeError:
            raise ValueError("`feature_cache` has to be an int, a dict or a sequence but is %r." % (interval,))
        if len(flags) != n:
            raise ValueError("`feature_cache` has %d entries but the scheduler runs %d evaluations (len(scheduler.timesteps))." % (len(flags), n))
    if flags:
        flags[0] = True
    co = [False] * n if cond_only is None else [bool(c) for c in cond_only]
    if len(co) != n:
        raise ValueError("feature_cache_plan: cond_only has %d entries for %d evaluations" % (len(co), n))
    halves_differ = False       # the most recent whole evaluation refreshed the conditional rows only
    for i in range(n):
        if not flags[i] and not co[i] and halves_differ:
            flags[i] = True
        if flags[i]:
            halves_differ = co[i]
    return flags


def feature_cache_spec(feature_cache, n_evals):
    """-> (flags or None, branch) of a `feature_cache=` argument: None (off), an int N >= 1, a dict {"interval": N or a sequence, "branch": k}
    or a sequence of one truthy / falsy entry per evaluation.  flags is None when no evaluation would run shallow (N = 1, all true): that is
    the plain run.  n_evals: the count or a callable returning it.  Raises ValueError for a bad interval, a branch outside 0..2, unknown dict
    keys or a wrong sequence length."""
    if feature_cache is None:
        return None, 0
    interval, branch = feature_cache, 0
    if isinstance(feature_cache, dict):
        extra = set(feature_cache) - {"interval", "branch"}
        if extra or "interval" not in feature_cache:
            raise ValueError("`feature_cache` dict takes the keys 'interval' and 'branch', got %r." % (sorted(feature_cache),))
        interval, branch = feature_cache["interval"], feature_cache.get("branch", 0)
    if isinstance(branch, bool) or not isinstance(branch, numbers.Integral) or not 0 <= branch <= 2:
        raise ValueError("`feature_cache` branch has to be 0, 1 or 2 but is %r." % (branch,))
    flags = feature_cache_plan(n_evals() if callable(n_evals) else n_evals, interval)
    return (None if all(flags) else flags), int(branch)


def pag_layer_mask(layers, layers_per_block=2):
    """-> the bit mask of `pag_applied_layers`: bit i = transformer block i in execution order, i.e. bits 0 .. 3L-1
    down_blocks.{0,1,2}.attentions.{0..L-1}, bit 3L the mid block, bits 3L+1 .. 6L+3 up_blocks.{1,2,3}.attentions.{0..L} (L =
    layers_per_block).  layers: one name or a list of "mid", "down", "up", "down.block_i", "up.block_i", "down.block_i.attentions_j",
    "up.block_i.attentions_j".  Raises ValueError for a name that selects no block (down.block_3 and up.block_0 have no attention), an
    unknown name or an empty list."""
    L = int(layers_per_block)
    if isinstance(layers, str):
        layers = [layers]
    try:
        names = list(layers)
    except TypeError:
        raise ValueError("`pag_applied_layers` has to be a name or a list of names but is %r." % (layers,))
    if not names:
        raise ValueError("`pag_applied_layers` selects no transformer block (empty list).")
    mask = 0
    for name in names:
        bad = ValueError("`pag_applied_layers`: %r selects no transformer block (mid, down, up, down.block_{0,1,2}[.attentions_j], "
                         "up.block_{1,2,3}[.attentions_j])." % (name,))
        if not isinstance(name, str):
            raise bad
        parts = name.split(".")
        if parts == ["mid"]:
            mask |= 1 << (3 * L)
            continue
        if parts[0] not in ("down", "up") or len(parts) > 3:
            raise bad
        down = parts[0] == "down"
        per = L if down else L + 1                    # attentions per block
        blocks = (0, 1, 2) if down else (1, 2, 3)     # the blocks that have attention
        base = (lambda i: i * L) if down else (lambda i: 3 * L + 1 + (i - 1) * (L + 1))
        if len(parts) == 1:
            sel = [(i, j) for i in blocks for j in range(per)]
        else:
            if not parts[1].startswith("block_") or not parts[1][6:].isdigit() or int(parts[1][6:]) not in blocks:
                raise bad
            i = int(parts[1][6:])
            if len(parts) == 2:
                sel = [(i, j) for j in range(per)]
            else:
                if not parts[2].startswith("attentions_") or not parts[2][11:].isdigit() or int(parts[2][11:]) >= per:
                    raise bad
                sel = [(i, int(parts[2][11:]))]
        for i, j in sel:
            mask |= 1 << (base(i) + j)
    return mask


def pag_plan(pag_scale, pag_adaptive_scale, timesteps):
    """-> the PAG scale of every evaluation (diffusers PAGMixin._get_pag_scale): pag_scale when pag_adaptive_scale == 0, else
    max(pag_scale - pag_adaptive_scale * (1000 - t_i), 0) with t_i the scheduler's timesteps.  Raises ValueError for a negative or non-finite
    scale."""
    try:
        s, a = float(pag_scale), float(pag_adaptive_scale)
    except (TypeError, ValueError):
        raise ValueError("`pag_scale` and `pag_adaptive_scale` have to be numbers but are %r and %r." % (pag_scale, pag_adaptive_scale))
    if not math.isfinite(s) or s < 0.0:
        raise ValueError("`pag_scale` has to be finite and >= 0 but is %r." % (pag_scale,))
    if not math.isfinite(a) or a < 0.0:
        raise ValueError("`pag_adaptive_scale` has to be finite and >= 0 but is %r." % (pag_adaptive_scale,))
    if a == 0.0:
        return [s for _ in timesteps]
    return [max(s - a * (1000.0 - float(t)), 0.0) for t in timesteps]


def sag_check(sag_scale, scheduler=None, latent_size=None, feature_cache=None, pag_table=None, tome_cfg=None, layers_per_block=2):
    """-> float(sag_scale), after the refusals of a run with self-attention guidance (the ones ladi_tryon_run makes, as ValueError).  0 checks
    nothing but the number.  scheduler: the scheduler object; latent_size: (h, w); pag_table: the PAG scales of the run or None; tome_cfg:
    the UNet's token-merging configuration or None."""
    try:
        s = float(sag_scale)
    except (TypeError, ValueError):
        raise ValueError("`sag_scale` has to be a number but is %r." % (sag_scale,))
    if not math.isfinite(s) or s < 0.0:
        raise ValueError("`sag_scale` has to be finite and >= 0 but is %r." % (sag_scale,))
    if s == 0.0:
        return s
    if feature_cache is not None:
        raise ValueError("`sag_scale` > 0 and `feature_cache` cannot be combined (a shallow evaluation does not run the mid block, whose "
                         "attention map SAG reads).")
    if pag_table is not None and any(p > 0.0 for p in pag_table):
        raise ValueError("`sag_scale` > 0 and `pag_scale` > 0 cannot be combined (both claim the sample group behind the conditional one).")
    if tome_cfg:
        from . import tome
        if tome.merged_mask(tome_cfg, layers_per_block) >> (3 * layers_per_block) & 1:
            raise ValueError("`sag_scale` > 0 with token merging in the mid block: the map would have merged tokens.")
    if isinstance(scheduler, (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, LMSDiscreteScheduler)):
        raise ValueError("`sag_scale` > 0 does not run with %s: the sigma-space schedulers rescale the model input, and pred_x0 / add_noise "
                         "do not describe them; use DDIM, PNDM, DPM-Solver++, LCM or TCD." % type(scheduler).__name__)
    if latent_size is not None and min(latent_size) < 5:
        raise ValueError("`sag_scale` > 0 needs latents of at least 5 x 5 (the blur's 4-pixel reflect padding) but they are %d x %d."
                         % tuple(latent_size))
    return s


def strength_first_step(strength, num_inference_steps):
    """-> first_step: the step of the schedule a run with `strength` starts at.  diffusers' get_timesteps arithmetic in Python float64:
    init_timestep = min(int(N * strength), N), first_step = N - init_timestep.  Raises ValueError for a strength outside [0, 1] or not finite,
    or one that leaves no step to run (init_timestep < 1)."""
    n = int(num_inference_steps)
    try:
        s = float(strength)
    except (TypeError, ValueError):
        raise ValueError("`strength` has to be a number in [0, 1] but is %r." % (strength,))
    if not math.isfinite(s) or s < 0.0 or s > 1.0:
        raise ValueError("`strength` has to be in [0, 1] but is %r." % (strength,))
    init_timestep = min(int(n * s), n)
    if init_timestep < 1:
        raise ValueError("`strength` = %r leaves no step to run with num_inference_steps = %d (int(%d * strength) < 1)." % (strength, n, n))
    return n - init_timestep


PRESERVE_MODES = {None: 0, "latents": 1, "pixels": 2, "both": 3}
MAX_FEATHER = 32.0


def preserve_spec(preserve_unmasked, mask_feather=0.0):
    """-> (mode_bits, sigma) of `preserve_unmasked=` / `mask_feather=`: bit 0 latents, bit 1 pixels (ladi_tryon_set_preserve).  Raises ValueError
    for an unknown mode, a feather that is negative, not finite or above 32, or a feather without a pixels mode."""
    if not (preserve_unmasked is None or isinstance(preserve_unmasked, str)) or preserve_unmasked not in PRESERVE_MODES:
        raise ValueError("`preserve_unmasked` has to be None, 'latents', 'pixels' or 'both' but is %r." % (preserve_unmasked,))
    bits = PRESERVE_MODES[preserve_unmasked]
    try:
        sigma = float(mask_feather)
    except (TypeError, ValueError):
        raise ValueError("`mask_feather` has to be a number in [0, %g] but is %r." % (MAX_FEATHER, mask_feather))
    if not math.isfinite(sigma) or sigma < 0.0 or sigma > MAX_FEATHER:
        raise ValueError("`mask_feather` has to be in [0, %g] but is %r." % (MAX_FEATHER, mask_feather))
    if sigma > 0.0 and not bits & 2:
        raise ValueError("`mask_feather` > 0 needs preserve_unmasked='pixels' or 'both' (it acts on the pixel composite only).")
    return bits, sigma


def feather_mask(mask, sigma):
    """the separable Gaussian blur of the pixel composite in torch fp32: mask [B, 1, H, W], radius ceil(3 sigma), weights normalised in
    float64, replicate border, rows then columns; a window of equal values returns that value exactly"""
    r = int(math.ceil(3.0 * sigma))
    k = torch.arange(-r, r + 1, dtype=torch.float64)
    wgt = torch.exp(-0.5 * k * k / (sigma * sigma))
    wgt = (wgt / wgt.sum()).to(device=mask.device, dtype=torch.float32)
    F = torch.nn.functional

    def one_pass(x, pad, shape):
        # a window of equal values returns that value itself, as the device kernel does: away from its edges the mask stays exactly 0 or 1
        xp = F.pad(x, pad, mode="replicate")
        size = (1, 2 * r + 1) if shape[-1] == -1 else (2 * r + 1, 1)
        hi, lo = F.max_pool2d(xp, size, stride=1), -F.max_pool2d(-xp, size, stride=1)
        return torch.where(lo == hi, lo, F.conv2d(xp, wgt.view(shape)))
    return one_pass(one_pass(mask.float(), (r, r, 0, 0), (1, 1, 1, -1)), (0, 0, r, r), (1, 1, -1, 1))


def rescale_noise_cfg(eps, eps_cond, phi):
    """guidance rescale: eps * (phi * std(eps_cond) / std(eps) + 1 - phi), per-sample unbiased stds, no epsilon"""
    dims = list(range(1, eps.ndim))
    return eps * (phi * (eps_cond.std(dim=dims, keepdim=True) / eps.std(dim=dims, keepdim=True)) + (1.0 - phi))


def numpy_to_pil(images):
    from PIL import Image
    if images.ndim == 3:
        images = images[None, ...]
    images = (images * 255).round().astype("uint8")
    return [Image.fromarray(im) for im in images]


class StableDiffusionTryOnePipeline:
    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, safety_checker=None, feature_extractor=None,
                 requires_safety_checker=False, emasc=None, emasc_int_layers=None, image_encoder=None):
        self.vae, self.text_encoder, self.tokenizer, self.unet, self.scheduler = vae, text_encoder, tokenizer, unet, scheduler
        self.emasc, self.emasc_int_layers = emasc, emasc_int_layers
        self.image_encoder = image_encoder      # NativeCLIPVisionEncoder (or None): encodes `ip_adapter_image` (encode_image)
        if getattr(scheduler.config, "steps_offset", 1) != 1:
            scheduler.config.steps_offset = 1          # tryon_pipe.py:74-86
        if getattr(scheduler.config, "skip_prk_steps", True) is False:
            scheduler.config.skip_prk_steps = True     # tryon_pipe.py:88-100
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self._tryon = None
        self.last_stage_ms = None
        self.trace_evals = 0          # > 0: the next fused runs record per-evaluation noise_pred / latents into self.last_trace
        self.lanes = None             # sample-group lanes of the fused loop's UNet forward (None: library default, LADI_UNET_LANES or 1)
        self._range_probe = None
        self._shallow_evals = None    # modular runs count here; fused runs ask the library

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' pipe.enable_freeu(s1, s2, b1, b2): forwarded to the UNet (NativeUNet.enable_freeu), where the state lives; the fused
        and the modular path both run it"""
        if not hasattr(self.unet, "enable_freeu"):
            raise ValueError("`enable_freeu` needs a UNet with enable_freeu (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        self.unet.enable_freeu(s1, s2, b1, b2)

    def set_pag_applied_layers(self, layers):
        """diffusers' pag_applied_layers: the transformer blocks whose self-attention the perturbed samples of `pag_scale` > 0 run with the
        identity map (pag_layer_mask's names; default "mid").  Forwarded to the UNet, where the state lives."""
        if not hasattr(self.unet, "set_pag_applied_layers"):
            raise ValueError("`set_pag_applied_layers` needs a UNet with set_pag_applied_layers (NativeUNet), the pipeline holds %s."
                             % type(self.unet).__name__)
        self.unet.set_pag_applied_layers(layers)

    def disable_freeu(self):
        if not hasattr(self.unet, "disable_freeu"):
            raise ValueError("`disable_freeu` needs a UNet with disable_freeu (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        self.unet.disable_freeu()

    # ---- token merging: the state lives in the UNet (NativeUNet.set_token_merging); the fused and the modular path both run it
    def apply_token_merging(self, ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False,
                            merge_mlp=False):
        """tomesd.apply_patch(pipe, ratio=...): in the transformer blocks of the first max_downsample levels the selected sub-layers run over
        T - int(T * ratio) tokens.  Holds for every later call until remove_token_merging(); ratio 0 is off.  use_rand draws the dst
        position of every 2 x 2 cell once per configuration from `seed` (tomesd redraws per block and evaluation)."""
        if not hasattr(self.unet, "set_token_merging"):
            raise ValueError("`apply_token_merging` needs the native UNet (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        self.unet.set_token_merging(ratio, max_downsample=max_downsample, sx=sx, sy=sy, use_rand=use_rand, seed=seed, merge_attn=merge_attn,
                                    merge_crossattn=merge_crossattn, merge_mlp=merge_mlp)

    def remove_token_merging(self):
        if not hasattr(self.unet, "remove_token_merging"):
            raise ValueError("`remove_token_merging` needs the native UNet (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        self.unet.remove_token_merging()

    @property
    def token_merging(self):
        """None while off, else the configuration as a dict"""
        return getattr(self.unet, "token_merging", None)

    # ---- LoRA: the state lives in the UNet (NativeUNet.load_lora_adapter / set_adapters), these are diffusers' pipeline-level names
    def _lora_unet(self, what):
        if not hasattr(self.unet, "load_lora_adapter"):
            raise ValueError("`%s` needs the native UNet (NativeUNet), the pipeline holds %s." % (what, type(self.unet).__name__))
        return self.unet

    def load_lora_weights(self, state_dict_or_path, adapter_name="default"):
        """diffusers' pipe.load_lora_weights: a LoRA state dict (PEFT, legacy diffusers or kohya keys) or a path to one (.safetensors where
        that module is installed, else a torch.save file).  The adapter is loaded and, as in diffusers, activated at weight 1.0 together
        with what was already active (after disable_lora(): together with the set that was put aside, which is enabled again).
        Text-encoder keys are not applied."""
        unet = self._lora_unet("load_lora_weights")
        sd = state_dict_or_path
        if not hasattr(sd, "items"):
            from . import lora
            sd = lora.load_file(sd)
        unet.load_lora_adapter(sd, adapter_name)
        # after disable_lora() the set that was put aside counts as "already active": loading re-enables it together with the new adapter
        # (set_adapters forgets the put-aside set, so it must not be lost here)
        active = unet.active_adapters or list(getattr(unet, "_lora_disabled", None) or [])
        try:
            unet.set_adapters([a[0] for a in active] + [adapter_name], [a[1] for a in active] + [1.0])
        except Exception:
            unet.delete_adapters(adapter_name)
            raise

    def set_adapters(self, adapter_names, adapter_weights=None):
        self._lora_unet("set_adapters").set_adapters(adapter_names, adapter_weights)

    def disable_lora(self):
        self._lora_unet("disable_lora").disable_lora()

    def enable_lora(self):
        self._lora_unet("enable_lora").enable_lora()

    def delete_adapters(self, adapter_names):
        self._lora_unet("delete_adapters").delete_adapters(adapter_names)

    def unload_lora_weights(self):
        """the plain weights back, every adapter freed"""
        unet = self._lora_unet("unload_lora_weights")
        unet.set_adapters([])
        unet.delete_adapters(unet.list_adapters())

    def get_active_adapters(self):
        return [a[0] for a in self._lora_unet("get_active_adapters").active_adapters]

    def get_list_adapters(self):
        return {"unet": self._lora_unet("get_list_adapters").list_adapters()}

    # ---- IP-Adapter image prompt: the state lives in the UNet (NativeUNet.load_ip_adapter / set_ip_adapter_scale)
    def _ip_unet(self, what):
        if not hasattr(self.unet, "load_ip_adapter"):
            raise ValueError("`%s` needs the native UNet (NativeUNet), the pipeline holds %s." % (what, type(self.unet).__name__))
        return self.unet

    def load_ip_adapter(self, state_dict_or_path, image_proj_dim_head=64):
        """diffusers' pipe.load_ip_adapter for the plain and the Plus adapter: a state dict in diffusers' {"image_proj", "ip_adapter"} layout
        or a path to one (ip_adapter.load_state).  A Plus file's Resampler is loaded with it (heads of image_proj_dim_head).  The call then
        takes the picture itself (`ip_adapter_image`, encoded by `pipe.image_encoder`) or `ip_adapter_image_embeds`."""
        self._ip_unet("load_ip_adapter").load_ip_adapter(state_dict_or_path, image_proj_dim_head)

    def unload_ip_adapter(self):
        self._ip_unet("unload_ip_adapter").unload_ip_adapter()

    def set_ip_adapter_scale(self, scale):
        """a number, or per-block scales as a dict / list in the names of set_pag_applied_layers (NativeUNet.set_ip_adapter_scale)"""
        self._ip_unet("set_ip_adapter_scale").set_ip_adapter_scale(scale)

    @property
    def image_encoder(self):
        """the vision encoder that turns `ip_adapter_image` into the adapter's input (NativeCLIPVisionEncoder; with `visual_projection.weight`
        in its weights for a plain adapter).  Settable; a new encoder drops the cached unconditional hidden states."""
        return getattr(self, "_image_encoder", None)

    @image_encoder.setter
    def image_encoder(self, enc):
        self._image_encoder = enc
        self._ip_uncond = None       # hidden_states[-2] of the zero pixel_values, one sample, computed on first use (encode_image)

    @staticmethod
    def _ip_image_tensor(image):
        """[B, 3, H, W] in [-1, 1] as it is; a PIL image or a list of PIL images of one size -> that layout, float32 (host arithmetic only)"""
        if isinstance(image, torch.Tensor):
            if image.dim() != 4 or image.shape[1] != 3:
                raise ValueError("`ip_adapter_image` has shape %s, expected [B, 3, H, W] in [-1, 1] (or PIL images)." % (tuple(image.shape),))
            return image
        import numpy as np
        ims = list(image) if isinstance(image, (list, tuple)) else [image]
        if not ims or not all(hasattr(im, "convert") for im in ims):
            raise ValueError("`ip_adapter_image` has to be a [B, 3, H, W] tensor in [-1, 1], a PIL image or a list of PIL images.")
        arr = [np.asarray(im.convert("RGB"), dtype=np.float32) for im in ims]
        if any(a.shape != arr[0].shape for a in arr):
            raise ValueError("the PIL images of `ip_adapter_image` have different sizes; resize them to one size first.")
        return torch.from_numpy(np.stack(arr)).permute(0, 3, 1, 2) / 127.5 - 1.0

    def encode_image(self, image, output_hidden_states=None):
        """diffusers' encode_image: -> (cond, uncond), what `ip_adapter_image_embeds` / `negative_ip_adapter_image_embeds` take.
        image: [B, 3, H, W] in [-1, 1] or PIL images.  It goes through warp.clip_preprocess at the encoder's image_size with the CLIP mean and
        std: the whole picture is resized (antialiased) to the square -- the pre-processing the reference applies to the in-shop cloth for
        the inversion adapter, NOT CLIPImageProcessor's shortest-edge resize plus centre crop.
        output_hidden_states (default: the loaded adapter is a Plus adapter): False -> cond = image_embeds [B, projection_dim], uncond =
        zeros_like (a plain adapter's input); True -> cond = hidden_states[-2] [B, T, hidden], uncond = hidden_states[-2] of zero
        pixel_values, computed for one sample once per encoder, cached on the pipeline and broadcast (a Plus adapter's input)."""
        enc = self.image_encoder
        if enc is None:
            raise ValueError("`encode_image` needs `pipe.image_encoder` (NativeCLIPVisionEncoder).")
        if output_hidden_states is None:
            output_hidden_states = bool(getattr(self.unet, "ip_adapter_is_plus", False))
        if not output_hidden_states and not getattr(enc, "projection_dim", 0):
            raise ValueError("`pipe.image_encoder` has no visual_projection (its weights lack visual_projection.weight): it cannot produce "
                             "image_embeds for a plain IP-Adapter.")
        from .warp import clip_preprocess
        px = clip_preprocess(self._ip_image_tensor(image), enc.cfg["image_size"])
        out = enc(px, output_hidden_states=bool(output_hidden_states))
        if not output_hidden_states:
            return out.image_embeds, torch.zeros_like(out.image_embeds)
        if getattr(self, "_ip_uncond", None) is None:
            self._ip_uncond = enc(torch.zeros_like(px[:1]), output_hidden_states=True).hidden_states[-2]
        cond = out.hidden_states[-2]
        return cond, self._ip_uncond.expand(cond.shape[0], -1, -1)

    @property
    def shallow_evals(self):
        """how many evaluations of the last run ran shallow (`feature_cache=`), after promotion (fused: ladi_tryon_shallow_evals)"""
        if self._shallow_evals is not None:
            return self._shallow_evals
        return _lib.load().ladi_tryon_shallow_evals(self._tryon) if self._tryon else None

    @property
    def range_probe(self):
        """a ladi_vton_amd.RangeProbe (default None = off: nothing is launched for it).  When set it is attached to unet, vae and emasc, for
        the fused and the modular path alike, and holds after every call the per-layer fp16 magnitudes / non-finite counts of that call
        (probe.report()).  The attachment follows the pipeline's modules: every call attaches it to the unet / vae / emasc the pipeline
        holds then, and takes it off a module that was replaced since.  With probe.raise_on_nonfinite = True a call that hands results to the host raises
        NativeError("fp16 range exceeded first at <name> ...") when a UNet / encoder / EMASC activation held an inf or NaN (a decoder
        overflow is left to the VAE's range-shift guard, which re-runs the batch)."""
        return self._range_probe

    @range_probe.setter
    def range_probe(self, probe):
        if self._range_probe is not None and self._range_probe is not probe:
            self._range_probe.detach()
        self._range_probe = probe
        if probe is not None:
            probe.attach_only(self.unet, self.vae, self.emasc)

    def _check_range_probe(self):
        """-> the name of the first UNet / encoder / EMASC point that left the fp16 range when the probe asks for an error, else None"""
        p = self._range_probe
        if p is None or not p.raise_on_nonfinite:
            return None
        name = p.first_nonfinite()
        return None if name is None or name.startswith(("decoder.", "post_quant_conv")) else name

    @staticmethod
    def _range_error(name):
        return _lib.NativeError("fp16 range exceeded first at %s (RangeProbe: inf / NaN in that activation; probe.report() has every layer)" % name)

    def to(self, *a, **k):
        return self

    @property
    def _execution_device(self):
        return torch.device("cuda", torch.cuda.current_device())

    # --- tryon_pipe.py:362-407 -------------------------------------------------------------------------------
    def check_inputs(self, prompt, height, width, callback_steps, negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError("Cannot forward both `negative_prompt` and `negative_prompt_embeds`.")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape, got "
                             f"{prompt_embeds.shape} != {negative_prompt_embeds.shape}.")

    # --- tryon_pipe.py:184-317 (text-encoder branch requires a real text_encoder/tokenizer) -------------------
    def _encode_prompt(self, prompt, device, num_images_per_prompt, do_cfg, negative_prompt=None, prompt_embeds=None,
                       negative_prompt_embeds=None):
        if prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("`prompt` given but the pipeline has no text_encoder/tokenizer; pass `prompt_embeds`.")
            ids = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                                 return_tensors="pt").input_ids
            prompt_embeds = self.text_encoder(ids.to(device))[0]
        prompt_embeds = prompt_embeds.to(device=device)
        B, L, D = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(B * num_images_per_prompt, L, D)
        if do_cfg and negative_prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds` when no text_encoder is attached.")
            toks = [""] * B if negative_prompt is None else ([negative_prompt] * B if isinstance(negative_prompt, str) else negative_prompt)
            ids = self.tokenizer(toks, padding="max_length", max_length=L, truncation=True, return_tensors="pt").input_ids
            negative_prompt_embeds = self.text_encoder(ids.to(device))[0]
        if do_cfg:
            neg = negative_prompt_embeds.to(device=device, dtype=prompt_embeds.dtype)
            neg = neg.repeat(1, num_images_per_prompt, 1).view(B * num_images_per_prompt, L, D)
            return prompt_embeds, neg
        return prompt_embeds, None

    @staticmethod
    def _validate_images(image, mask_image):
        # diffusers prepare_mask_and_masked_image tensor branch
        if not isinstance(image, torch.Tensor) or not isinstance(mask_image, torch.Tensor):
            raise TypeError("`image` and `mask_image` must be torch tensors")
        if image.ndim != 4 or mask_image.ndim != 4:
            raise ValueError("`image` and `mask_image` must be 4-D batches")
        if image.shape[-2:] != mask_image.shape[-2:] or image.shape[0] != mask_image.shape[0]:
            raise ValueError("Image and Mask must have the same spatial dimensions and batch size")
        if image.min() < -1 or image.max() > 1:
            raise ValueError("Image should be in [-1, 1] range")
        if mask_image.min() < 0 or mask_image.max() > 1:
            raise ValueError("Mask should be in [0, 1] range")

    def _draw(self, shape, generator, dtype, device):
        """diffusers randn_tensor: one draw of the whole batch, or -- for a LIST of generators (tryon_pipe.py:443-455,463-470) -- one
        [1, ...] draw per sample from that sample's generator"""
        if isinstance(generator, (list, tuple)):
            if len(generator) != shape[0]:
                raise ValueError("You have passed a list of generators of length %d, but requested an effective batch size of %d."
                                 % (len(generator), shape[0]))
            parts = [torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device, dtype=dtype).to(device) for g in generator]
            return torch.cat(parts, dim=0).to(torch.float32)
        gdev = generator.device if generator is not None else device
        return torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device=device, dtype=torch.float32)

    def decode_latents(self, latents, intermediate_features=None):
        z = latents / self.vae.config.scaling_factor
        if intermediate_features:
            image = self.vae.decode(z, intermediate_features=intermediate_features, int_layers=self.emasc_int_layers).sample
        else:
            image = self.vae.decode(z).sample
        image = (image / 2 + 0.5).clamp(0, 1)
        return image.cpu().permute(0, 2, 3, 1).float().numpy()

    @torch.no_grad()
    def __call__(self, image, mask_image, pose_map, warped_cloth, prompt=None, height=None, width=None, num_inference_steps=50,
                 guidance_scale=7.5, negative_prompt=None, num_images_per_prompt=1, eta=0.0, prompt_embeds=None,
                 negative_prompt_embeds=None, generator=None, latents=None, output_type="pil", return_dict=True, callback=None,
                 callback_steps=1, cloth_cond_rate=1.0, no_pose=False, cloth_input_type="warped", fused=True, noise=None,
                 use_graph=True, guidance_rescale=0.0, strength=1.0, init_image=None, init_latents=None, init_is_noisy=False,
                 feature_cache=None, preserve_unmasked=None, mask_feather=0.0, pag_scale=0.0, pag_adaptive_scale=0.0,
                 ip_adapter_image_embeds=None, negative_ip_adapter_image_embeds=None, sag_scale=0.0, ip_adapter_image=None):
        """tryon_pipe.py's __call__.  `guidance_scale`: a float, a sequence with one scale per evaluation (len(scheduler.timesteps); PNDM: steps
        + 1) or a callable f(i, n_evals) -- see guidance_interval.  Classifier-free guidance is on if any scale is > 1; an evaluation whose scale
        is <= 1 then runs the UNet over the conditional samples only.  `guidance_rescale` (rescale_noise_cfg's phi, [0, 1]) acts on the CFG
        evaluations.  `height` / `width`: any multiple of 8, as the reference's check_inputs.  Latent sides that are not
        multiples of 8 (e.g. 640x480 -> 80x60) run diffusers' `forward_upsample_size` arithmetic on both the fused and the modular path.

        `strength` < 1 starts the run at step first_step = N - min(int(N * strength), N) of the N-step schedule from an init instead of from
        noise at step 0, and runs only the tail.  The init is `init_latents` (fp32 [B, 4, hs, ws] in the loop's latent space, e.g.
        `pipe.last_latents` of an earlier run or what a step callback received) or `init_image` ([B, 3, Hi, Wi] in [-1, 1], sides multiples of
        8: encoded with the pipeline's VAE, posterior mode * scaling_factor, no extra RNG draw); another size than the run's is resampled
        bilinearly.  The start latents are k_x * init + k_n * noise with the scheduler's add_noise coefficients at timesteps[first_step] and the
        noise of `latents=` / RNG draw #2; `init_is_noisy=True` takes the init as the loop's latents at that timestep unchanged (resume).
        Everything indexed per evaluation (a guidance schedule, the callback's i, scheduler.timesteps, the cloth cut-off of `cloth_cond_rate`)
        refers to the tail.  PNDM restarts as a fresh PLMS run over the tail (tail steps + 1 evaluations, at least 2 steps).  strength = 1.0
        ignores a given init and is the plain run.  LCMScheduler and TCDScheduler run the tail of their N-step list too, like every other
        scheduler here; diffusers' set_timesteps(strength=), which spaces the N steps anew over the shortened range, is not used.

        `eta` goes to DDIMScheduler.step and, as its gamma, to TCDScheduler.step (there it has to be in [0, 1]); no other scheduler reads it.
        Few-step sampling: LCMScheduler / TCDScheduler (1 .. original_inference_steps evaluations) and timestep_spacing="trailing" on
        DDIM, Euler and Euler-ancestral (1 .. 1000).  Their step() draws one batch-shaped fp32 tensor at every evaluation but the last (TCD
        with eta = 0: none), after the pipeline's three draws; the fused path makes exactly those draws up front, so both paths agree for a
        seed.

        `feature_cache` (DeepCache on the full-resolution level; None = off): an int N (every N-th evaluation runs the whole UNet, the others
        only its outermost layers on the deep features the last whole one cached), a dict {"interval": N, "branch": k} (k = 0, 1, 2: how many
        layers of the first down block, and as many more of the last up block, a shallow evaluation runs; default 0) or a sequence of one
        truthy (whole) / falsy (shallow) entry per evaluation.  Evaluation 0 is always whole; N = 1 or an all-true sequence is the plain run.
        See feature_cache_plan for the one promotion rule; the cloth cut-off, a callback's edit of the latents and PNDM's double evaluation
        reuse the cache as it is.  Needs the native UNet.  `pipe.shallow_evals` counts the shallow evaluations of the last run.

        `preserve_unmasked` (None = off) hands the region outside `mask_image` back unchanged.  "latents" is diffusers' 4-channel inpaint
        rule: after every scheduler update the latent pixels whose whole 8x8 footprint is unmasked are replaced by the known image noised to
        the next timestep, k_x z0 + k_n noise with the scheduler's add_noise coefficients at timesteps[i + 1], and by z0 after the last
        evaluation; z0 is the posterior mode of vae.encode(image) times scaling_factor (one more encode, no extra RNG draw) and the noise is
        that of `latents=` / RNG draw #2, also with `strength` < 1.  Scheduler state is not blended; a callback sees the blended latents.
        "pixels" composites the decoded picture over the input image, M g + (1 - M) p with the binarised mask M, or its Gaussian blur of
        `mask_feather` pixels sigma (0 .. 32); where M is 0 or 1 the pixel is p or g bit for bit, in the float and the uint8 output alike.
        "both" does both.  `mask_feather` needs a pixels mode.

        `pag_scale` > 0 is perturbed-attention guidance (diffusers PAGMixin): every evaluation also runs a perturbed copy of the conditional
        samples, whose self-attention in the blocks of `set_pag_applied_layers` (default the mid block) is the identity map, and the
        prediction becomes u + g (c - u) + s (c - p), or c + s (c - p) without classifier-free guidance; `guidance_rescale` acts on that
        sum.  `pag_adaptive_scale` > 0 lowers the scale with the timestep, s_i = max(pag_scale - pag_adaptive_scale * (1000 - t_i), 0); an
        evaluation with s_i = 0 runs without the perturbed samples.  Needs the native UNet; not together with `feature_cache`.  0 is the
        plain run bit for bit.

        `ip_adapter_image_embeds` is the image prompt of a loaded IP-Adapter (load_ip_adapter): [B, E] or [B, 1, E] image embeddings, or
        diffusers' one-element list holding [2B, 1, E] with the negatives first.  `negative_ip_adapter_image_embeds` defaults to zeros.  Every
        cross-attention then adds scale * softmax(q k_ip^T / 8) v_ip over the projected image tokens (set_ip_adapter_scale; fused and modular
        path alike).  With a Plus adapter the embeddings are hidden states of the image encoder, [B, T, E], or the one-element list holding
        [2B, T, E] with the negatives first.  `ip_adapter_image` is the picture itself instead ([B, 3, H, W] in [-1, 1] or PIL images, one per
        sample of the batch): `pipe.image_encoder` encodes it (encode_image: whole-picture resize, not a centre crop) into what the loaded
        adapter takes -- image_embeds for a plain adapter, whose encoder needs a visual_projection of the adapter's width, hidden_states[-2]
        for a Plus adapter.  It cannot be combined with `ip_adapter_image_embeds`.  None for both is the plain run.

        `sag_scale` > 0 is self-attention guidance (diffusers StableDiffusionSAGPipeline, whose default is 0.75): every evaluation reads the
        self-attention map of the mid block, blurs the regions of its own x0 estimate that receive more than average attention (9 x 9
        Gaussian, sigma 1), re-noises them with the predicted noise and steers away from the prediction d for that degraded input:
        e + sag_scale * (b - d), b the unconditional prediction under classifier-free guidance, else the conditional one;
        `guidance_rescale` acts on the whole sum.  One more forward over B samples per evaluation.  Needs the native UNet, DDIM / PNDM /
        DPM-Solver++ / LCM / TCD and latents of at least 5 x 5; not together with `feature_cache`, `pag_scale` > 0 or token merging in the mid
        block (sag_check).  0 is the plain run bit for bit."""
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds)
        if image is None:
            raise ValueError("`image` input cannot be undefined.")
        if mask_image is None:
            raise ValueError("`mask_image` input cannot be undefined.")
        if cloth_input_type not in ("warped", "none"):
            raise ValueError(f"Invalid cloth_input_type {cloth_input_type}")
        # num_images_per_prompt = k repeats every prompt k times (tryon_pipe.py:259-260,309-310) and sizes the latents for B * k samples
        # (:659); the reference concatenates image-derived tensors (pose map, warped cloth) unrepeated (:724-729), so the only inputs it
        # can run are image batches that already hold B * k samples -- the same rule applies here (shape checks below)
        if not isinstance(num_images_per_prompt, int) or num_images_per_prompt < 1:
            raise ValueError("num_images_per_prompt must be a positive integer")
        if isinstance(self.scheduler, TCDScheduler) and not 0.0 <= float(eta) <= 1.0:
            raise ValueError("`eta` is TCDScheduler's gamma and has to be in [0, 1] but is %r." % (eta,))
        first_step = strength_first_step(strength, num_inference_steps)
        preserve = preserve_spec(preserve_unmasked, mask_feather)
        if init_image is not None and init_latents is not None:
            raise ValueError("Cannot forward both `init_image` and `init_latents`.")
        if first_step > 0:
            if init_image is None and init_latents is None:
                raise ValueError("`strength` < 1 needs `init_image` or `init_latents` to start from.")
            if not isinstance(self.scheduler, FUSED_SCHEDULERS):
                raise ValueError("`strength` < 1 needs one of this package's schedulers (set_timesteps(..., first_step=)).")
        # the scheduler's own keyword stays out of a plain run's call (first_step == 0: today's set_timesteps(n) / (n, device=))
        ts_kw = {"first_step": first_step} if first_step > 0 else {}

        def n_evals():
            self.scheduler.set_timesteps(num_inference_steps, **ts_kw)
            return len(self.scheduler.timesteps)
        if first_step > 0:
            n_evals()      # a first_step the scheduler cannot start at (a PNDM tail of one step) fails here, before any work
        g_table, guidance_scale, do_cfg = guidance_plan(guidance_scale, n_evals, guidance_rescale)
        pag_plan(pag_scale, pag_adaptive_scale, ())          # negative / non-finite scales fail here, before any work
        pag_table = None
        if float(pag_scale) > 0.0:
            if not hasattr(self.unet, "set_pag_applied_layers"):
                raise ValueError("`pag_scale` needs the native UNet (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
            if feature_cache is not None:
                raise ValueError("`pag_scale` > 0 and `feature_cache` cannot be combined (the cache has no third sample group).")
            if getattr(self.unet, "token_merging", None):
                from . import tome
                tome.check_pag_layers(self.unet.token_merging, self.unet.pag_applied_layers, self.unet.cfg["layers_per_block"])
            n_evals()
            pag_table = pag_plan(pag_scale, pag_adaptive_scale, self.scheduler.timesteps)
            if not any(s > 0.0 for s in pag_table):
                pag_table = None
        sag_scale = sag_check(sag_scale, self.scheduler, (height // self.vae_scale_factor, width // self.vae_scale_factor), feature_cache,
                              pag_table, getattr(self.unet, "token_merging", None), getattr(self.unet, "cfg", {}).get("layers_per_block", 2))
        if sag_scale > 0.0 and not isinstance(self.unet, NativeUNet):
            raise ValueError("`sag_scale` needs the native UNet (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        fc_flags, fc_branch = feature_cache_spec(feature_cache, n_evals)
        if feature_cache is not None and not isinstance(self.unet, NativeUNet):
            raise ValueError("`feature_cache` needs the native UNet (NativeUNet), the pipeline holds %s." % type(self.unet).__name__)
        self._shallow_evals = None
        device = self._execution_device
        pe, neg = self._encode_prompt(prompt, device, num_images_per_prompt, do_cfg, negative_prompt, prompt_embeds, negative_prompt_embeds)
        B = pe.shape[0]
        ip = None
        if ip_adapter_image is not None:
            # every refusal comes before the encoder runs: nothing is launched for a call that is not going to happen
            if ip_adapter_image_embeds is not None or negative_ip_adapter_image_embeds is not None:
                raise ValueError("Cannot forward both `ip_adapter_image` and `ip_adapter_image_embeds` / `negative_ip_adapter_image_embeds`.")
            ip_unet = self._ip_unet("ip_adapter_image")
            info = ip_unet.ip_adapter_info
            if info is None:
                raise ValueError("`ip_adapter_image` needs a loaded IP-Adapter (load_ip_adapter).")
            enc = self.image_encoder
            if enc is None:
                raise ValueError("`ip_adapter_image` needs `pipe.image_encoder` (NativeCLIPVisionEncoder) to encode the picture.")
            plus = ip_unet.ip_adapter_is_plus
            if plus and enc.cfg["hidden"] != info[1]:
                raise ValueError("`pipe.image_encoder` has hidden states of width %d, the loaded Plus adapter takes %d." % (enc.cfg["hidden"], info[1]))
            if not plus and not getattr(enc, "projection_dim", 0):
                raise ValueError("`pipe.image_encoder` has no visual_projection (its weights lack visual_projection.weight), which the loaded "
                                 "plain IP-Adapter needs: it takes image_embeds.")
            if not plus and enc.projection_dim != info[1]:
                raise ValueError("`pipe.image_encoder` projects to %d, the loaded adapter takes embeddings of width %d." % (enc.projection_dim, info[1]))
            picture = self._ip_image_tensor(ip_adapter_image)
            if picture.shape[0] != B:
                raise ValueError("`ip_adapter_image` has batch %d, the prompt embeddings have %d." % (picture.shape[0], B))
            ip = tuple(t.to(device=device, dtype=torch.float16).contiguous() for t in self.encode_image(picture, plus))
        elif ip_adapter_image_embeds is not None:
            from . import ip_adapter
            ip_unet = self._ip_unet("ip_adapter_image_embeds")
            info = ip_unet.ip_adapter_info
            if info is None:
                raise ValueError("`ip_adapter_image_embeds` needs a loaded IP-Adapter (load_ip_adapter).")
            ip_pos, ip_neg = ip_adapter.split_embeds(ip_adapter_image_embeds, negative_ip_adapter_image_embeds, B, do_cfg,
                                                     seq=ip_unet.ip_adapter_is_plus)
            if ip_pos.shape[-1] != info[1]:
                raise ValueError("`ip_adapter_image_embeds` has width %d, the loaded adapter takes %d." % (ip_pos.shape[-1], info[1]))
            ip_pos = ip_pos.to(device=device, dtype=torch.float16).contiguous()
            ip_neg = ip_neg.to(device=device, dtype=torch.float16).contiguous() if ip_neg is not None else torch.zeros_like(ip_pos)
            ip = (ip_pos, ip_neg)
        elif negative_ip_adapter_image_embeds is not None:
            raise ValueError("`negative_ip_adapter_image_embeds` without `ip_adapter_image_embeds`.")
        self._validate_images(image, mask_image)
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        # RNG draws in pipeline order (cloth posterior, initial latents, masked-image posterior)
        if noise is None:
            n_cloth = self._draw((B, 4, h, w), generator, pe.dtype, device) if cloth_input_type == "warped" else None
            n_lat = latents.to(device=device, dtype=torch.float32) if latents is not None else self._draw((B, 4, h, w), generator, pe.dtype, device)
            n_mask = self._draw((B, 4, h, w), generator, pe.dtype, device)
        else:
            n_cloth, n_lat, n_mask = [t.to(device=device, dtype=torch.float32).contiguous() if t is not None else None for t in noise]
        if self._range_probe is not None:
            self._range_probe.attach_only(self.unet, self.vae, self.emasc)     # the modules of THIS call (one may have been replaced)
            self._range_probe.reset()
        init = self._prepare_init(init_image, init_latents, B, device) if first_step > 0 else None
        native = isinstance(self.unet, NativeUNet) and isinstance(self.vae, NativeVAE) and (self.emasc is None or isinstance(self.emasc, NativeEMASC))
        # only DDIMScheduler.step and TCDScheduler.step (its gamma) take eta (the modular path passes it to no other scheduler); a negative
        # one stays on the modular path
        ddim_eta = float(eta) if isinstance(self.scheduler, (DDIMScheduler, TCDScheduler)) else 0.0
        can_fuse = (fused and native and isinstance(self.scheduler, FUSED_SCHEDULERS) and ddim_eta >= 0.0
                    and (not self.emasc or list(self.emasc_int_layers or []) == [1, 2, 3, 4, 5]))
        if can_fuse:
            # Euler / Euler-ancestral / DDIM with eta > 0 step() draw one batch-shaped fp32 noise tensor per step after the three draws above:
            # the fused path makes the same draws up front, in the same generator order (Euler's are unused, as in diffusers without churn)
            step_noise = None
            few_step = isinstance(self.scheduler, (LCMScheduler, TCDScheduler))
            if isinstance(self.scheduler, (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler)) or (ddim_eta > 0.0 and not few_step):
                draws = [self._draw((B, 4, h, w), generator, torch.float32, device) for _ in range(int(num_inference_steps) - first_step)]
                if not isinstance(self.scheduler, EulerDiscreteScheduler):
                    step_noise = torch.stack(draws).contiguous()
            elif isinstance(self.scheduler, LCMScheduler) or (isinstance(self.scheduler, TCDScheduler) and ddim_eta > 0.0):
                # LCM / TCD with eta > 0 draw at every evaluation but the last: exactly those evaluations - 1 draws, and one slab per
                # evaluation for the runtime, the last zero-filled and not drawn (its table row has c_n = 0: never read)
                draws = [self._draw((B, 4, h, w), generator, torch.float32, device) for _ in range(int(num_inference_steps) - first_step - 1)]
                if draws:
                    step_noise = torch.stack(draws + [torch.zeros_like(draws[0])]).contiguous()
            if callback is not None:
                self.scheduler.set_timesteps(num_inference_steps, device=device, **ts_kw)    # the callback's t, as on the modular path
            images = self._run_fused(image, mask_image, pose_map, warped_cloth if cloth_input_type == "warped" else None, pe, neg,
                                     n_cloth, n_lat, n_mask, height, width, num_inference_steps, guidance_scale, cloth_cond_rate,
                                     no_pose, use_graph, step_noise=step_noise, eta=ddim_eta, callback=callback,
                                     callback_steps=callback_steps, guidance_table=g_table, guidance_rescale=guidance_rescale,
                                     init_latents=init, first_step=first_step, init_is_noisy=init_is_noisy,
                                     feature_cache=(fc_flags, fc_branch), preserve=preserve, pag_table=pag_table, ip=ip, sag_scale=sag_scale)
            # prepare_mask_and_masked_image binarises the caller's mask in place; keep that side effect
            mask_image[mask_image < 0.5] = 0
            mask_image[mask_image >= 0.5] = 1
        else:
            images = self._run_modular(image, mask_image, pose_map, warped_cloth if cloth_input_type == "warped" else None, pe, neg,
                                       n_cloth, n_lat, n_mask, height, width, num_inference_steps, guidance_scale, cloth_cond_rate,
                                       no_pose, eta, generator, callback, callback_steps, guidance_table=g_table,
                                       guidance_rescale=guidance_rescale, init_latents=init, first_step=first_step,
                                       init_is_noisy=init_is_noisy, feature_cache=(fc_flags, fc_branch), preserve=preserve,
                                       pag_table=pag_table, ip=ip, sag_scale=sag_scale)
        if output_type == "pil":
            images = numpy_to_pil(images)
        if not return_dict:
            return (images, None)
        return SimpleNamespace(images=images, nsfw_content_detected=None)

    def _prepare_init(self, init_image, init_latents, B, device):
        """-> the init of a strength < 1 run as fp32 [B, 4, hs, ws] latents on `device`.  init_image: the posterior MODE of the pipeline's own
        vae.encode times scaling_factor (no RNG draw, so the pipeline's three draws keep their order; later diffusers releases sample it)"""
        if init_latents is not None:
            if not isinstance(init_latents, torch.Tensor) or init_latents.ndim != 4 or tuple(init_latents.shape[:2]) != (B, 4) \
                    or min(init_latents.shape[2:]) < 1:
                raise ValueError("`init_latents` has to be a [%d, 4, hs, ws] tensor but has shape %s."
                                 % (B, tuple(getattr(init_latents, "shape", ()))))
            return init_latents.to(device=device, dtype=torch.float32).contiguous()
        if not isinstance(init_image, torch.Tensor) or init_image.ndim != 4 or tuple(init_image.shape[:2]) != (B, 3):
            raise ValueError("`init_image` has to be a [%d, 3, Hi, Wi] tensor but has shape %s." % (B, tuple(getattr(init_image, "shape", ()))))
        if init_image.shape[2] % 8 or init_image.shape[3] % 8 or min(init_image.shape[2:]) < 8:
            raise ValueError("`init_image` sides have to be multiples of 8 but are %d and %d." % tuple(init_image.shape[2:]))
        if init_image.min() < -1 or init_image.max() > 1:
            raise ValueError("`init_image` should be in [-1, 1] range")
        mode = self.vae.encode(init_image.to(device))[0].latent_dist.mode()
        return (self.vae.config.scaling_factor * mode.float()).contiguous()

    # -------------------------------------------------------------------------------------------------------
    def _run_fused(self, image, mask_image, pose_map, cloth, pe, neg, n_cloth, n_lat, n_mask, H, W, steps, guidance, ccr, no_pose,
                   use_graph, return_device=False, out_uint8=False, lanes=None, step_noise=None, eta=0.0, callback=None, callback_steps=1,
                   guidance_table=None, guidance_rescale=0.0, init_latents=None, first_step=0, init_is_noisy=False, feature_cache=None,
                   preserve=None, pag_table=None, ip=None, sag_scale=0.0):
        """ip: (embeds, negative embeds), fp16 [B, E] device tensors each (ladi_tryon_set_ip_adapter), or [B, T, E] hidden states for a Plus
        adapter (ladi_tryon_set_ip_adapter_seq); None = no image prompt.
        return_device: hand back the device tensor (no host copy); out_uint8: the batch as uint8 [B,H,W,3] = numpy_to_pil's
        (images * 255).round() computed by the decode epilogue (ladi_tryon_run_u8); lanes: sample-group lanes of the UNet forward;
        step_noise: fp32 [steps, B, 4, h, w], the per-step noise of EulerAncestralDiscreteScheduler and of DDIM with eta > 0
        (ladi_tryon_set_step_noise; LCM and TCD with eta > 0 too, their last slab unread); eta: DDIM's eta or TCD's gamma
        (ladi_tryon_set_eta); guidance_table: one scale per evaluation, replaces `guidance` (ladi_tryon_set_guidance_schedule; None = off); guidance_rescale: phi of ladi_tryon_set_guidance_rescale;
        callback / callback_steps: called as callback(i, self.scheduler.timesteps[i], latents) after every evaluation i with
        i % callback_steps == 0, latents an fp32 [B, 4, h, w] device tensor whose in-place edits the loop takes over
        (ladi_tryon_set_step_callback).  An exception in the callback aborts the run and is re-raised here.  When the decode's fp16-range
        guard re-runs the batch (below), the whole loop runs again and the callback sees every step a second time.
        init_latents / first_step / init_is_noisy (ladi_tryon_set_init): start at step first_step > 0 of the `steps`-step schedule from the fp32
        [B, 4, hs, ws] init_latents (None or first_step = 0: off).  The run then has the tail's evaluations: step_noise, guidance_table, the
        callback's i and the cloth cut-off of `ccr` all refer to them.
        feature_cache: (flags, branch) of feature_cache_spec, one flag per evaluation before promotion (ladi_tryon_set_feature_cache does the
        promotion); None or flags None = off.
        preserve: (mode_bits, feather sigma) of preserve_spec (ladi_tryon_set_preserve); None = off.
        pag_table: one PAG scale per evaluation (pag_plan; ladi_tryon_set_pag); None = off.
        sag_scale: the self-attention guidance scale (ladi_tryon_set_sag); 0 = off."""
        lib = _lib.load()
        if self._tryon is None:
            self._tryon = lib.ladi_tryon_create(self.unet.h, self.vae.h, self.emasc.h if self.emasc else None)
            if not self._tryon:
                raise _lib.NativeError("ladi_tryon_create failed: " + _lib.last_error())
        dev = self._execution_device
        dt = torch.float16 if image.dtype == torch.float16 else torch.float32
        B = pe.shape[0]
        # the C ABI takes raw device pointers: every shape the kernels assume is checked here (the reference fails in torch.cat at
        # tryon_pipe.py:724-729 for the same mistakes)
        h8, w8 = H // 8, W // 8
        for name, t, shp in (("image", image, (B, 3, H, W)), ("mask_image", mask_image, (B, 1, H, W)),
                             ("warped_cloth", cloth, (B, 3, H, W)), ("cloth posterior noise", n_cloth, (B, 4, h8, w8)),
                             ("latents", n_lat, (B, 4, h8, w8)), ("masked-image posterior noise", n_mask, (B, 4, h8, w8))):
            if t is not None and tuple(t.shape) != shp:
                raise ValueError("%s has shape %s, expected %s (batch from prompt_embeds, size from height/width)" % (name, tuple(t.shape), shp))
        if pose_map.dim() != 4 or pose_map.shape[0] != B or tuple(pose_map.shape[2:]) != (H, W):
            raise ValueError("pose_map has shape %s, expected (%d, P, %d, %d)" % (tuple(pose_map.shape), B, H, W))
        if neg is not None and tuple(neg.shape) != tuple(pe.shape):
            raise ValueError("negative_prompt_embeds shape %s != prompt_embeds shape %s" % (tuple(neg.shape), tuple(pe.shape)))
        keep = [t.to(device=dev, dtype=dt).contiguous() if t is not None else None for t in (image, mask_image, pose_map, cloth)]
        pe16 = pe.to(device=dev, dtype=torch.float16).contiguous()
        neg16 = neg.to(device=dev, dtype=torch.float16).contiguous() if neg is not None else None
        n_cloth, n_lat, n_mask = [t.to(device=dev, dtype=torch.float32).contiguous() if t is not None else None for t in (n_cloth, n_lat, n_mask)]
        inp = TryOnInputs()
        inp.batch, inp.height, inp.width, inp.in_dtype = B, H, W, dtype_code(keep[0])
        inp.image_dev, inp.mask_image_dev, inp.pose_map_dev = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
        inp.warped_cloth_dev = keep[3].data_ptr() if keep[3] is not None else None
        inp.pose_channels = keep[2].shape[1]
        inp.prompt_embeds_dev = pe16.data_ptr()
        inp.negative_prompt_embeds_dev = neg16.data_ptr() if neg16 is not None else None
        inp.L = pe16.shape[1]
        inp.noise_cloth_dev = n_cloth.data_ptr() if n_cloth is not None else None
        inp.noise_latents_dev, inp.noise_masked_dev = n_lat.data_ptr(), n_mask.data_ptr()
        inp.num_inference_steps, inp.guidance_scale = int(steps), float(guidance)
        inp.scheduler = self.scheduler.kind
        # tryon_pipe.py:654,718 in the reference's own float64 arithmetic: first evaluation index i with i >= steps - (1 - rate) * steps
        # (a run that starts at first_step: the tail's step count in the same formula, as the reference loop handed diffusers' truncated
        # num_inference_steps would compute it)
        first_step = int(first_step) if init_latents is not None else 0
        tail = int(steps) - first_step
        ccs = (1 - ccr) * tail
        inp.cloth_zero_from_eval = min(max(0, math.ceil(tail - ccs)), 1 << 30)
        inp.no_pose, inp.use_graph = int(bool(no_pose)), int(bool(use_graph))
        ac = self.scheduler.alphas_cumprod.to("cpu", torch.float32).contiguous()
        inp.alphas_cumprod_host = ac.data_ptr()
        images = torch.empty((B, H, W, 3), dtype=torch.uint8 if out_uint8 else torch.float32, device=dev)
        self.last_latents = torch.empty((B, 4, H // 8, W // 8), dtype=torch.float32, device=dev)
        tr = None
        if self.trace_evals > 0:
            tr = torch.zeros((2, self.trace_evals, B, h8 * w8, 4), dtype=torch.float32, device=dev)
            check(lib.ladi_tryon_set_trace(self._tryon, ptr(tr[0]), ptr(tr[1]), self.trace_evals), "ladi_tryon_set_trace")
        else:
            check(lib.ladi_tryon_set_trace(self._tryon, None, None, 0), "ladi_tryon_set_trace")
        if step_noise is not None:
            if tuple(step_noise.shape[1:]) != (B, 4, h8, w8) or step_noise.shape[0] < tail:
                raise ValueError("step noise has shape %s, expected (%d, %d, 4, %d, %d)" % (tuple(step_noise.shape), tail, B, h8, w8))
            step_noise = step_noise.to(device=dev, dtype=torch.float32).contiguous()
            check(lib.ladi_tryon_set_step_noise(self._tryon, ptr(step_noise), step_noise.shape[0]), "ladi_tryon_set_step_noise")
        else:
            check(lib.ladi_tryon_set_step_noise(self._tryon, None, 0), "ladi_tryon_set_step_noise")
        check(lib.ladi_tryon_set_eta(self._tryon, float(eta)), "ladi_tryon_set_eta")
        if first_step > 0:
            if init_latents.ndim != 4 or tuple(init_latents.shape[:2]) != (B, 4):
                raise ValueError("init latents have shape %s, expected (%d, 4, hs, ws)" % (tuple(init_latents.shape), B))
            init_latents = init_latents.to(device=dev, dtype=torch.float32).contiguous()
            check(lib.ladi_tryon_set_init(self._tryon, ptr(init_latents), init_latents.shape[2], init_latents.shape[3], first_step,
                                          int(bool(init_is_noisy))), "ladi_tryon_set_init")
        else:
            check(lib.ladi_tryon_set_init(self._tryon, None, 0, 0, 0, 0), "ladi_tryon_set_init")
        if guidance_table is not None:
            gt = (ctypes.c_float * len(guidance_table))(*guidance_table)
            check(lib.ladi_tryon_set_guidance_schedule(self._tryon, gt, len(guidance_table)), "ladi_tryon_set_guidance_schedule")
        else:
            check(lib.ladi_tryon_set_guidance_schedule(self._tryon, None, 0), "ladi_tryon_set_guidance_schedule")
        check(lib.ladi_tryon_set_guidance_rescale(self._tryon, float(guidance_rescale)), "ladi_tryon_set_guidance_rescale")
        fc_flags, fc_branch = feature_cache if feature_cache is not None else (None, 0)
        if fc_flags is not None:
            ff = (ctypes.c_ubyte * len(fc_flags))(*[1 if f else 0 for f in fc_flags])
            check(lib.ladi_tryon_set_feature_cache(self._tryon, ff, len(fc_flags), int(fc_branch)), "ladi_tryon_set_feature_cache")
        else:
            check(lib.ladi_tryon_set_feature_cache(self._tryon, None, 0, 0), "ladi_tryon_set_feature_cache")
        if pag_table is not None:
            pt = (ctypes.c_float * len(pag_table))(*pag_table)
            check(lib.ladi_tryon_set_pag(self._tryon, pt, len(pag_table)), "ladi_tryon_set_pag")
        else:
            check(lib.ladi_tryon_set_pag(self._tryon, None, 0), "ladi_tryon_set_pag")
        check(lib.ladi_tryon_set_sag(self._tryon, float(sag_scale)), "ladi_tryon_set_sag")
        if float(sag_scale) > 0.0:
            self.unet._sag_last = ((2 if neg16 is not None else 1) * B, h8, w8)      # sag_map()'s defaults: the run's context batch
        p_bits, p_sigma = preserve if preserve is not None else (0, 0.0)
        check(lib.ladi_tryon_set_preserve(self._tryon, int(p_bits), float(p_sigma)), "ladi_tryon_set_preserve")
        if ip is not None:
            for t in ip:
                if t.dim() not in (2, 3) or t.shape != ip[0].shape or t.shape[0] != B or t.dtype != torch.float16 or not t.is_contiguous():
                    raise ValueError("image embeddings have shape %s (%s), expected a contiguous fp16 [%d, E] (Plus adapter: [%d, T, E])"
                                     % (tuple(t.shape), t.dtype, B, B))
            if ip[0].dim() == 3:      # hidden states of a Plus adapter: the run puts them through the UNet's Resampler
                check(lib.ladi_tryon_set_ip_adapter_seq(self._tryon, ptr(ip[0]), ptr(ip[1]), int(ip[0].shape[1])), "ladi_tryon_set_ip_adapter_seq")
            else:
                check(lib.ladi_tryon_set_ip_adapter(self._tryon, ptr(ip[0]), ptr(ip[1])), "ladi_tryon_set_ip_adapter")
        else:
            check(lib.ladi_tryon_set_ip_adapter(self._tryon, None, None), "ladi_tryon_set_ip_adapter")
        self._shallow_evals = None
        cb_error = []
        cb_latents = trampoline = None
        if callback is not None:
            cb_latents = torch.empty((B, 4, h8, w8), dtype=torch.float32, device=dev)
            timesteps = self.scheduler.timesteps

            def _step(_user, i):
                try:
                    callback(i, timesteps[i], cb_latents)
                    return 0
                except BaseException as e:     # noqa: B902  (re-raised after the native call returns)
                    cb_error.append(e)
                    return 1
            trampoline = _lib.STEP_CALLBACK(_step)     # referenced until the callback is switched off below
            check(lib.ladi_tryon_set_step_callback(self._tryon, trampoline, None, int(callback_steps), ptr(cb_latents)),
                  "ladi_tryon_set_step_callback")
        # the fused loop rewrites the UNet's cross-attention K/V cache (and its image context) behind the shim's back
        self.unet._ctx_key = None
        self.unet._ip_key = None
        if lanes is not None or self.lanes is not None:
            check(lib.ladi_tryon_set_lanes(self._tryon, int(lanes if lanes is not None else self.lanes)), "ladi_tryon_set_lanes")
        native_run = lib.ladi_tryon_run_u8 if out_uint8 else lib.ladi_tryon_run

        def run(what):
            rc = native_run(self._tryon, ctypes.byref(inp), ptr(images), ptr(self.last_latents), stream_ptr())
            if cb_error:
                raise cb_error[0]
            check(rc, what)
        try:
            run("ladi_tryon_run")
            bad = None if return_device else self._check_range_probe()
            if bad is not None:
                # NaN latents also trip the decoder's guard: take its flag so that the next run is not refused for this one (the automatic
                # range shift it raises stays; it only adds decoder head-room)
                lib.ladi_tryon_poll_overflow(self._tryon)
                raise self._range_error(bad)
            if not return_device:
                # results go to the host: this is the synchronisation point anyway, so the decode's fp16-range guard is asked now (a run
                # decodes once and queues its flag; no host round trip inside the run).  An overflow raised the automatic range shift: run the
                # batch again (a step callback then sees every step a second time).  With return_device the flag is examined by the next call
                # instead (or by check_overflow()), which fails loudly rather than hand out a bad batch silently.
                for _ in range(2):
                    po = lib.ladi_tryon_poll_overflow(self._tryon)
                    if po == 0:
                        break
                    if po < 0:
                        raise _lib.NativeError("ladi_tryon_poll_overflow: " + _lib.last_error())
                    run("ladi_tryon_run (re-run at a larger range shift)")
                else:
                    if lib.ladi_tryon_poll_overflow(self._tryon) != 0:
                        raise _lib.NativeError("VAE decode: activations exceed the fp16 range even at range shift 8")
        finally:
            if trampoline is not None:
                check(lib.ladi_tryon_set_step_callback(self._tryon, _lib.NO_STEP_CALLBACK, None, 1, None), "ladi_tryon_set_step_callback")
        if tr is not None:   # [evals, B, 4, h, w] like the reference's noise_pred / latents (tryon_pipe.py:732-740)
            nchw = tr.view(2, self.trace_evals, B, h8, w8, 4).permute(0, 1, 2, 5, 3, 4)
            self.last_trace = dict(noise_pred=nchw[0].contiguous(), latents=nchw[1].contiguous())
        if return_device:
            return images
        out = images.cpu().numpy()  # the reference's only sync point (tryon_pipe.py:358)
        ms = (ctypes.c_float * 3)()
        if lib.ladi_tryon_stage_ms(self._tryon, ms) == 0:
            self.last_stage_ms = list(ms)
        return out

    def _sag_degrade(self, latents, e_b, m, sqrt_a, sqrt_1ma):
        """steps 2-3 of self-attention guidance through the kernel the fused loop runs (ladi_op_sag_degrade): latents fp32 [B, 4, h, w], the
        base prediction e_b (fp16 values), the SAG mask m uint8 [B, hm, wm] -> the degraded latents fp32 [B, 4, h, w] (fp16 values, as the
        UNet input holds them)"""
        B, _, h, w = latents.shape
        lat = latents.float().permute(0, 2, 3, 1).contiguous()
        eb = e_b.permute(0, 2, 3, 1).to(torch.float16).contiguous()
        out = torch.empty((B, h, w, 4), dtype=torch.float16, device=latents.device)
        m = m.contiguous()
        check(_lib.load().ladi_op_sag_degrade(ptr(lat), ptr(eb), 4, ptr(m), B, h, w, m.shape[1], m.shape[2], sqrt_a, sqrt_1ma, 1.0, None, ptr(out),
                                              4, 4, stream_ptr()), "ladi_op_sag_degrade")
        return out.permute(0, 3, 1, 2).float().contiguous()

    def check_overflow(self):
        """True if the last fused run's decode left the fp16 range (its images are invalid; the automatic range shift has been raised, so running
        the batch again gives the result).  For callers that keep results on the device (return_device=True): waits for the run to finish."""
        if not self._tryon:
            return False
        po = _lib.load().ladi_tryon_poll_overflow(self._tryon)
        if po < 0:
            raise _lib.NativeError("ladi_tryon_poll_overflow: " + _lib.last_error())
        return po == 1

    def cond_only_evals(self):
        """how many evaluations of the last fused run ran cond-only (ladi_tryon_cond_only_evals)"""
        return _lib.load().ladi_tryon_cond_only_evals(self._tryon) if self._tryon else None

    def lib_lanes(self):
        """sample-group lanes the last fused run used"""
        return _lib.load().ladi_tryon_lanes(self._tryon) if self._tryon else None

    def __del__(self):
        if getattr(self, "_tryon", None):
            _lib.load().ladi_tryon_destroy(self._tryon)
            self._tryon = None

    # -------------------------------------------------------------------------------------------------------
    def _run_modular(self, image, mask_image, pose_map, cloth, pe, neg, n_cloth, n_lat, n_mask, H, W, steps, guidance, ccr, no_pose, eta,
                     generator, callback, callback_steps, guidance_table=None, guidance_rescale=0.0, init_latents=None, first_step=0,
                     init_is_noisy=False, feature_cache=None, preserve=None, pag_table=None, ip=None, sag_scale=0.0):
        F = torch.nn.functional
        dev = self._execution_device
        do_cfg = neg is not None
        sf = self.vae.config.scaling_factor
        ehs = torch.cat([neg, pe]) if do_cfg else pe
        # PAG: the context of the whole run is [neg ; pe ; pe] (or [pe ; pe]); every evaluation runs its own rows of it
        ehs_pag = torch.cat([ehs, pe]) if pag_table is not None else None
        # the image prompt follows the context row for row: [neg ; pos], [pos], with PAG one more pos
        ip_c = ip_all = ip_pag = None
        if ip is not None:
            ip_c = ip[0]
            ip_all = torch.cat([ip[1], ip[0]]) if do_cfg else ip[0]
            ip_pag = torch.cat([ip_all, ip[0]])

        def ipkw(t):
            return {"ip_image_embeds": t} if ip is not None else {}
        mask_image[mask_image < 0.5] = 0
        mask_image[mask_image >= 0.5] = 1
        mask = mask_image.to(dev)
        masked_image = image.to(dev).float() * (mask < 0.5)
        pose = F.interpolate(pose_map.to(dev).float(), size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
        if no_pose:
            pose = torch.zeros_like(pose)
        cloth_lat = None
        if cloth is not None:
            cloth_lat = sf * self.vae.encode(cloth.to(dev))[0].latent_dist.sample(noise=n_cloth).float()
        first_step = int(first_step) if init_latents is not None else 0
        if first_step > 0:
            # strength: the tail of the schedule from k_x * resample(init) + k_n * noise (the scheduler's add_noise at the first timestep), or
            # from the init itself (init_is_noisy); `steps` below is the tail's count, as diffusers hands the loop its truncated one
            self.scheduler.set_timesteps(steps, device=dev, first_step=first_step)
            timesteps = self.scheduler.timesteps
            steps = int(steps) - first_step
            x0 = init_latents.to(device=dev, dtype=torch.float32)
            if tuple(x0.shape[2:]) != (H // 8, W // 8):
                x0 = F.interpolate(x0, size=(H // 8, W // 8), mode="bilinear", align_corners=False)
            latents = x0 if init_is_noisy else self.scheduler.add_noise(x0, n_lat.to(dev), timesteps[0])
        else:
            self.scheduler.set_timesteps(steps, device=dev)
            timesteps = self.scheduler.timesteps
            latents = n_lat * self.scheduler.init_noise_sigma
        ccs = (1 - ccr) * steps
        p_bits, p_sigma = preserve if preserve is not None else (0, 0.0)
        if p_bits & 1:
            # preserve-unmasked, latents: z0 (the posterior mode: no RNG draw) and the latent pixels whose whole 8x8 footprint is unmasked
            z0 = (sf * self.vae.encode(image.to(dev))[0].latent_dist.mode().float()).contiguous()
            keep = F.max_pool2d(mask.float(), 8) < 0.5
            keep_noise = n_lat.to(dev)
        mask_lat = F.interpolate(mask.float(), size=(H // 8, W // 8))
        enc, feats = self.vae.encode(masked_image)
        masked_lat = sf * enc.latent_dist.sample(noise=n_mask).float()
        inter = None
        if self.emasc:
            inter = [feats[i] for i in self.emasc_int_layers]
            inter = self.emasc(inter)
            inter = mask_features(inter, mask_image.to(dev))
        if do_cfg:
            mask_lat = torch.cat([mask_lat] * 2)
            masked_lat = torch.cat([masked_lat] * 2)
            pose = torch.cat([torch.zeros_like(pose), pose])
            if cloth_lat is not None:
                cloth_lat = torch.cat([torch.zeros_like(cloth_lat), cloth_lat])
        extra = {}
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        if "eta" in params:
            extra["eta"] = eta
        if "generator" in params:
            extra["generator"] = generator
        B = latents.shape[0]
        # feature cache: the plan after promotion; a cond-only evaluation of a CFG run then keeps the whole context and runs the conditional
        # samples as rows [B, 2B) of it, so that it meets the rows of the cache the CFG evaluations wrote (as the fused loop does)
        fc_flags, fc_branch = feature_cache if feature_cache is not None else (None, 0)
        if fc_flags is not None:
            co = [do_cfg and guidance_table is not None and not guidance_table[i] > 1.0 for i in range(len(timesteps))]
            fc_flags = feature_cache_plan(len(timesteps), fc_flags, co)
            self._shallow_evals = sum(1 for f in fc_flags if not f)
        else:
            self._shallow_evals = 0
        for i, t in enumerate(timesteps):
            g_i = guidance_table[i] if guidance_table is not None else guidance
            # a cond-only evaluation of a CFG run (scale <= 1): the B conditional samples and the conditional context alone
            cfg_i = do_cfg and (guidance_table is None or g_i > 1.0)
            x = torch.cat([latents] * 2) if cfg_i else latents
            if cloth_lat is not None and i >= (steps - ccs):
                cloth_lat = torch.zeros_like(cloth_lat)
            x = self.scheduler.scale_model_input(x, t)
            parts = [x, mask_lat, masked_lat, pose] + ([cloth_lat] if cloth_lat is not None else [])
            if do_cfg and not cfg_i:
                parts = [x] + [p[B:] for p in parts[1:]]
            s_i = pag_table[i] if pag_table is not None else 0.0
            if s_i > 0.0:      # the perturbed group: the conditional group's rows once more
                parts = [torch.cat([p, p[-B:]]) for p in parts]
            x = torch.cat([p.float() for p in parts], dim=1)
            if pag_table is not None:
                ng = 2 if do_cfg else 1
                eps = self.unet(x, t, encoder_hidden_states=ehs_pag, sample0=B if do_cfg and not cfg_i else 0, pag_first=ng * B,
                                **ipkw(ip_pag)).sample.float()
                if s_i > 0.0:
                    eps, ep = eps[:-B], eps[-B:]
            elif fc_flags is not None:
                eps = self.unet(x, t, encoder_hidden_states=ehs, feature_cache="capture" if fc_flags[i] else "reuse", cache_branch=fc_branch,
                                sample0=B if do_cfg and not cfg_i else 0, **ipkw(ip_all)).sample.float()
            elif sag_scale > 0.0:
                # self-attention guidance, steps 1-4: the first forward leaves the SAG map; the base group is the first B rows of this
                # evaluation (uncond under CFG, else cond); sag_degrade gives the degraded latents; the second forward runs them with the
                # base group's other channels, context rows and image tokens, and leaves the map alone
                whole = cfg_i or not do_cfg
                ctx, ipx = (ehs if whole else pe), (ip_all if whole else ip_c)
                self.unet.set_sag_capture(True)
                try:
                    eps = self.unet(x, t, encoder_hidden_states=ctx, **ipkw(ipx)).sample.float()
                finally:
                    self.unet.set_sag_capture(False)
                e_b = eps[:B]
                a_t = float(self.scheduler.alphas_cumprod[int(round(float(t)))].float())
                xd = self._sag_degrade(latents, e_b, self.unet.sag_map(n=B, latent_size=(H // 8, W // 8))[1], math.sqrt(a_t), math.sqrt(1.0 - a_t))
                x2 = torch.cat([xd] + [p[:B].float() for p in parts[1:]], dim=1)
                e_d = self.unet(x2, t, encoder_hidden_states=ctx[:B], **ipkw(ipx[:B] if ipx is not None else None)).sample.float()
            else:
                whole = cfg_i or not do_cfg
                eps = self.unet(x, t, encoder_hidden_states=ehs if whole else pe, **ipkw(ip_all if whole else ip_c)).sample.float()
            if cfg_i:
                eu, et = eps.chunk(2)
                eps = eu + g_i * (et - eu)
                if s_i > 0.0:
                    eps = eps + s_i * (et - ep)
                if sag_scale > 0.0:
                    eps = eps + sag_scale * (eu - e_d)
                if guidance_rescale > 0.0:
                    eps = rescale_noise_cfg(eps, et, guidance_rescale)
            elif s_i > 0.0:
                eps = eps + s_i * (eps - ep)
            elif sag_scale > 0.0:
                eps = eps + sag_scale * (eps - e_d)
            latents = self.scheduler.step(eps, t, latents, **extra).prev_sample
            if p_bits & 1:
                known = self.scheduler.add_noise(z0, keep_noise, timesteps[i + 1]) if i + 1 < len(timesteps) else z0
                latents = torch.where(keep, known.to(latents.dtype), latents)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        self.last_latents = latents
        images = self.decode_latents(latents, inter)
        if p_bits & 2:
            # preserve-unmasked, pixels: the decoded picture over the input image, a select where the (feathered) mask is 0 or 1
            m = feather_mask(mask, p_sigma) if p_sigma > 0.0 else mask.float()
            m = m.permute(0, 2, 3, 1).cpu()
            g = torch.from_numpy(images)
            p = (image.to(dev).float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu()
            images = torch.where(m == 0, p, torch.where(m == 1, g, m * g + (1 - m) * p)).numpy()
        bad = self._check_range_probe()
        if bad is not None:
            raise self._range_error(bad)
        return images
