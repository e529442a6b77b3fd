"""LoRA state dicts for the native UNet: key normalisation (pure Python, no GPU) and reading a checkpoint from disk.

An adapter reaches the library (ladi_unet_lora_load, include/ladi_native.h) as `<module>.lora_down.weight`, `<module>.lora_up.weight` and an
optional `<module>.alpha`, `<module>` being the diffusers name of a conv / linear of the UNet.  normalize_state_dict brings the three
formats in circulation to that form:

  PEFT              [base_model.model.][unet.]<module>.lora_A[.<adapter>].weight / .lora_B[.<adapter>].weight
  legacy diffusers  [unet.]<module>.lora.down.weight / .lora.up.weight, and the attention-processor form
                    [unet.]<...attnN>.processor.to_q_lora.down.weight (to_out_lora is <...attnN>.to_out.0)
  kohya             lora_unet_<module with _ for .>.lora_down.weight / .lora_up.weight / .alpha

Not supported, by design: text-encoder LoRA (such keys are separated and reported, never applied), DoRA and
bias factors (they raise), a per-call `cross_attention_kwargs={"scale": ..}` and an unmerged execution mode.
"""
import re
import warnings
from collections import OrderedDict

import torch

from . import configs

_PREFIXES = ("base_model.model.", "unet.")
_TE_PREFIXES = ("lora_te", "text_encoder")


class NormalizedLoRA(OrderedDict):
    """{module: (down, up, alpha)}; .text_encoder_keys: the keys of the source that belong to a text encoder (not applied)"""
    text_encoder_keys = ()


def target_modules(cfg):
    """the diffusers names of every conv / linear of a UNet of configuration cfg (what a LoRA factor pair may be attached to)"""
    return [k[:-len(".weight")] for k, s in configs.unet_shapes(cfg).items() if k.endswith(".weight") and len(s) >= 2]


def _strip(key):
    changed = True
    while changed:
        changed = False
        for p in _PREFIXES:
            if key.startswith(p):
                key, changed = key[len(p):], True
    return key


_SUFFIXES = (
    # (regex on the stripped key, role)
    (re.compile(r"^(?P<m>.+)\.lora_A(\.[^.]+)?\.weight$"), "down"),
    (re.compile(r"^(?P<m>.+)\.lora_B(\.[^.]+)?\.weight$"), "up"),
    (re.compile(r"^(?P<m>.+)\.lora\.down\.weight$"), "down"),
    (re.compile(r"^(?P<m>.+)\.lora\.up\.weight$"), "up"),
    (re.compile(r"^(?P<m>.+)\.lora_down\.weight$"), "down"),
    (re.compile(r"^(?P<m>.+)\.lora_up\.weight$"), "up"),
    (re.compile(r"^(?P<m>.+)\.alpha$"), "alpha"),
)
_PROCESSOR = re.compile(r"^(?P<a>.+)\.processor\.(?P<p>to_q|to_k|to_v|to_out)_lora\.(?P<r>down|up)\.weight$")


def normalize_state_dict(sd, module_names):
    """sd: a LoRA state dict in PEFT, legacy diffusers or kohya form (module docstring); module_names: the UNet's target modules
    (target_modules(cfg)).  Returns a NormalizedLoRA {module: (down, up, alpha)} of float32 tensors: down [r, in] or [r, in, k, k] (conv
    factors keep their 4-D shape), up [out, r] (a [out, r, 1, 1] factor is the same thing), alpha a float (the rank where the source has none).
    kohya names are resolved by a table built from module_names, never by guessing where the dots were.  Text-encoder keys are collected in
    .text_encoder_keys and reported with a warning.  DoRA keys, bias factors, unknown modules, a factor without its partner and factors whose
    ranks disagree raise ValueError."""
    names = set(module_names)
    kohya = {}
    for m in module_names:
        if kohya.setdefault(m.replace(".", "_"), m) != m:
            raise ValueError("module names %r and %r collide once '.' is written as '_'" % (kohya[m.replace(".", "_")], m))
    parts, te = OrderedDict(), []
    for key, val in sd.items():
        low = key.lower()
        bare = key[len("base_model.model."):] if key.startswith("base_model.model.") else key
        if bare.startswith(_TE_PREFIXES):
            te.append(key)
            continue
        if "dora_scale" in low or "lora_magnitude_vector" in low:
            raise ValueError("DoRA key %r: weight-decomposed adapters are not supported" % key)
        if low.endswith(".bias") or ".lora_bias" in low or low.endswith("lora_b.bias"):
            raise ValueError("bias key %r: LoRA bias factors are not supported (biases are not targets)" % key)
        k = _strip(key)
        mod = role = None
        if k.startswith("lora_unet_"):
            for suf, r in ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha")):
                if k.endswith(suf):
                    flat, role = k[len("lora_unet_"):-len(suf)], r
                    mod = kohya.get(flat)
                    if mod is None:
                        raise ValueError("kohya key %r names no conv / linear of this UNet" % key)
                    break
        else:
            pm = _PROCESSOR.match(k)
            if pm:
                mod, role = pm.group("a") + "." + ("to_out.0" if pm.group("p") == "to_out" else pm.group("p")), pm.group("r")
            else:
                for rx, r in _SUFFIXES:
                    m = rx.match(k)
                    if m:
                        mod, role = m.group("m"), r
                        break
        if mod is None:
            raise ValueError("key %r is not a LoRA factor this library knows (PEFT, legacy diffusers or kohya form)" % key)
        if mod not in names:
            raise ValueError("key %r: module %r is not a conv / linear of this UNet" % (key, mod))
        slot = parts.setdefault(mod, {})
        if role in slot:
            raise ValueError("module %r has two %s entries (second: %r)" % (mod, role, key))
        slot[role] = val
    out = NormalizedLoRA()
    for mod, slot in parts.items():
        if "down" not in slot or "up" not in slot:
            raise ValueError("module %r: the %s factor is missing" % (mod, "down" if "down" not in slot else "up"))
        down = torch.as_tensor(slot["down"]).detach().to("cpu", torch.float32).contiguous()
        up = torch.as_tensor(slot["up"]).detach().to("cpu", torch.float32)
        if down.dim() not in (2, 4) or up.dim() not in (2, 4) or (up.dim() == 4 and tuple(up.shape[2:]) != (1, 1)):
            raise ValueError("module %r: factors of shapes %r / %r are not LoRA factors" % (mod, tuple(down.shape), tuple(up.shape)))
        up = up.reshape(up.shape[0], up.shape[1]).contiguous()
        if down.shape[0] != up.shape[1]:
            raise ValueError("module %r: down has rank %d, up has rank %d" % (mod, down.shape[0], up.shape[1]))
        alpha = float(torch.as_tensor(slot["alpha"]).reshape(-1)[0]) if "alpha" in slot else float(down.shape[0])
        out[mod] = (down, up, alpha)
    out.text_encoder_keys = tuple(te)
    if te:
        warnings.warn("%d text-encoder LoRA keys are not applied (text-encoder LoRA is out of scope): %s .." % (len(te), te[0]))
    return out


def to_library_keys(norm):
    """NormalizedLoRA -> the flat {key: tensor} ladi_unet_lora_load takes"""
    flat = OrderedDict()
    for mod, (down, up, alpha) in norm.items():
        flat[mod + ".lora_down.weight"] = down
        flat[mod + ".lora_up.weight"] = up
        flat[mod + ".alpha"] = torch.tensor([alpha], dtype=torch.float32)
    return flat


def load_file(path):
    """a LoRA checkpoint from disk: .safetensors where that module is importable, else torch.load"""
    if str(path).endswith(".safetensors"):
        try:
            from safetensors.torch import load_file as st_load
        except ImportError:
            raise RuntimeError("%s: reading .safetensors needs the safetensors module, which is not installed; convert the file with torch.save" % path)
        return st_load(str(path))
    sd = torch.load(str(path), map_location="cpu")
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd
