"""IP-Adapter checkpoints for the native UNet: diffusers' `{"image_proj": {...}, "ip_adapter": {...}}` layout -> the keys
ladi_unet_ip_adapter_load takes (include/ladi_native.h "IP-Adapter image prompt"), and the per-block scale list of set_ip_adapter_scale.

Supported: the plain adapter, whose image projection is `ImageProjection` (proj: Linear [N * cross_dim, E], norm: LayerNorm per token),
and the Plus adapter, whose image projection is the tencent-ailab `Resampler` in its ORIGINAL key layout (RESAMPLER_TOP, resampler_keys:
what the `image_proj` of a released ip-adapter-plus file holds; diffusers' internally renamed keys are not taken).  That layout and the
Resampler's arithmetic (resampler.py) are written from memory of the IP-Adapter package, which is not a dependency, and were not checked
against it.  A complete Resampler dict comes back under `image_proj.<original key>`; an incomplete one is refused, as are FaceID
projections and lists of several adapters.  Tokens computed elsewhere go in through NativeUNet.__call__(ip_tokens=) /
ladi_unet_set_ip_tokens.
"""
import re

import torch

from . import lora
from .pipeline import pag_layer_mask

PROCESSOR = ".transformer_blocks.0.attn2.processor."
PROJ_KEYS = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")


def block_prefixes(layers_per_block=2):
    """the transformer blocks in execution order (entry i = scale i of ladi_unet_set_ip_scale = bit i of the PAG mask)"""
    L = int(layers_per_block)
    return (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] + ["mid_block.attentions.0"] +
            ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)])


def numbered_order(layers_per_block=2):
    """THE table of the numbered checkpoint keys: entry k is the block that "<2k+1>.to_k_ip.weight" belongs to.  diffusers numbers the
    attention processors in `unet.attn_processors` order -- down_blocks, then up_blocks, then mid_block, attn1 (even) before attn2 (odd)
    inside a block -- so the mid block is the last index.  diffusers is not a dependency of this package: the order is written from
    memory of its loader (_convert_ip_adapter_attn_to_diffusers), not checked against it."""
    L = int(layers_per_block)
    return (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] +
            ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)] + ["mid_block.attentions.0"])


def _split(sd):
    """-> (image_proj dict, ip_adapter dict) from the nested layout or from flat keys with those prefixes"""
    if isinstance(sd, (list, tuple)):
        raise ValueError("a list of IP-Adapters (several adapters at once) is not supported: load one adapter")
    if not hasattr(sd, "items"):
        raise ValueError("an IP-Adapter state dict has to be a dict but is %s" % type(sd).__name__)
    if "image_proj" in sd and "ip_adapter" in sd and hasattr(sd["image_proj"], "items"):
        return dict(sd["image_proj"]), dict(sd["ip_adapter"])
    proj, ada = {}, {}
    for k, v in sd.items():
        if k.startswith("image_proj."):
            proj[k[len("image_proj."):]] = v
        elif k.startswith("ip_adapter."):
            ada[k[len("ip_adapter."):]] = v
        elif PROCESSOR in k:
            ada[k] = v
        else:
            raise ValueError("unexpected IP-Adapter key %r (want image_proj.*, ip_adapter.* or <block>%sto_k_ip / to_v_ip.weight)" % (k, PROCESSOR))
    return proj, ada


RESAMPLER_TOP = ("latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias")
RESAMPLER_LAYER = ("0.norm1.weight", "0.norm1.bias", "0.norm2.weight", "0.norm2.bias", "0.to_q.weight", "0.to_kv.weight", "0.to_out.weight",
                   "1.0.weight", "1.0.bias", "1.1.weight", "1.3.weight")


def resampler_keys(depth):
    """every key of a Resampler of `depth` layers, original layout"""
    return list(RESAMPLER_TOP) + ["layers.%d.%s" % (i, k) for i in range(int(depth)) for k in RESAMPLER_LAYER]


def check_resampler(proj, dim_head=None):
    """Is `proj` (an image_proj dict) a complete Resampler of consistent shapes?  -> dict(N, E, dim, depth, inner, out_dim), or ValueError.
    The library checks the same again (and the limits that need dim_head, when it is not given here); this one needs no library and names
    what a partial or renamed checkpoint lacks."""
    refuse = ("this is a Resampler ('plus') image projection, but %s; a complete one in the original key layout is loaded with the adapter, "
              "else compute the image tokens elsewhere and pass them as ip_tokens= (ladi_unet_set_ip_tokens)")
    depth = 0
    while "layers.%d.0.to_q.weight" % depth in proj:
        depth += 1
    want = set(resampler_keys(max(depth, 1)))
    missing, extra = sorted(want - set(proj)), sorted(set(proj) - want)
    if missing:
        raise ValueError(refuse % ("it lacks %d of %d keys, e.g. %r" % (len(missing), len(want), missing[0])))
    if extra:
        raise ValueError(refuse % ("it has the unexpected key %r (diffusers' renamed Resampler keys are not taken)" % extra[0]))
    shp = {k: tuple(v.shape) for k, v in proj.items()}
    lat = shp["latents"]
    if len(lat) != 3 or lat[0] != 1:
        raise ValueError(refuse % ("latents has shape %s, expected [1, N, dim]" % (lat,)))
    N, dim = lat[1], lat[2]
    if len(shp["proj_in.weight"]) != 2 or len(shp["proj_out.weight"]) != 2 or len(shp["layers.0.0.to_q.weight"]) != 2:
        raise ValueError(refuse % "proj_in / proj_out / to_q are not matrices")
    E, out_dim, inner = shp["proj_in.weight"][1], shp["proj_out.weight"][0], shp["layers.0.0.to_q.weight"][0]
    expect = {"proj_in.weight": (dim, E), "proj_in.bias": (dim,), "proj_out.weight": (out_dim, dim), "proj_out.bias": (out_dim,),
              "norm_out.weight": (out_dim,), "norm_out.bias": (out_dim,)}
    for i in range(depth):
        p = "layers.%d." % i
        ff = shp[p + "1.1.weight"][0]
        for k in ("0.norm1", "0.norm2", "1.0"):
            expect[p + k + ".weight"] = expect[p + k + ".bias"] = (dim,)
        expect.update({p + "0.to_q.weight": (inner, dim), p + "0.to_kv.weight": (2 * inner, dim), p + "0.to_out.weight": (dim, inner),
                       p + "1.1.weight": (ff, dim), p + "1.3.weight": (dim, ff)})
    for k, s in expect.items():
        if shp[k] != s:
            raise ValueError(refuse % ("%s has shape %s, expected %s" % (k, list(shp[k]), list(s))))
    if not 1 <= N <= 64:
        raise ValueError(refuse % ("it has %d latents (image tokens), outside [1, 64]" % N))
    if E % 8 or dim % 8 or out_dim % 8:
        raise ValueError(refuse % ("its widths E = %d, dim = %d, out_dim = %d are not all multiples of 8" % (E, dim, out_dim)))
    if dim_head is not None:
        if dim_head not in (64, 80, 96, 128):
            raise ValueError(refuse % ("dim_head %r is not one of 64, 80, 96, 128" % (dim_head,)))
        if inner % dim_head:
            raise ValueError(refuse % ("its attention width %d is no multiple of dim_head %d" % (inner, dim_head)))
    return dict(N=N, E=E, dim=dim, depth=depth, inner=inner, out_dim=out_dim)


def load_state(path_or_dict, layers_per_block=2):
    """-> {library key: tensor}.  Accepts diffusers' nested dict, a flat dict or file (.safetensors where that module is installed, else
    torch.load) with the prefixes image_proj. / ip_adapter., numbered keys "<2k+1>.to_k_ip.weight" (numbered_order) and module-named keys
    "<block>.transformer_blocks.0.attn2.processor.to_k_ip.weight" as they are.  The image projection is the plain one (PROJ_KEYS) or a
    complete Resampler (check_resampler), returned under image_proj.<original key>.  Raises ValueError for what is out of scope."""
    sd = path_or_dict if hasattr(path_or_dict, "items") or isinstance(path_or_dict, (list, tuple)) else lora.load_file(path_or_dict)
    proj, ada = _split(sd)
    plus = any(k.startswith(("latents", "proj_in.", "proj_out.", "layers.")) or "perceiver" in k for k in proj)
    if plus:
        check_resampler(proj)
    if any(k.startswith(("proj.0.", "proj.2.", "proj.3.")) for k in proj) or any("lora" in k for k in ada):
        raise ValueError("this is a FaceID adapter (MLP image projection / LoRA processors), which is not supported; its tokens cannot go "
                         "through ip_tokens= either when it carries LoRA weights")
    if not plus and set(proj) != set(PROJ_KEYS):
        raise ValueError("image_proj has the keys %s, expected %s (the plain ImageProjection)" % (sorted(proj), sorted(PROJ_KEYS)))
    order = numbered_order(layers_per_block)
    out = {"image_proj." + k: proj[k] for k in (sorted(proj) if plus else PROJ_KEYS)}
    for k, v in ada.items():
        m = re.fullmatch(r"(\d+)\.(to_[kv]_ip)\.weight", k)
        if m:
            idx = int(m.group(1))
            if idx % 2 == 0 or idx // 2 >= len(order):
                raise ValueError("ip_adapter key %r: the index has to be odd and below %d (one cross-attention per transformer block)"
                                 % (k, 2 * len(order)))
            key = order[idx // 2] + PROCESSOR + m.group(2) + ".weight"
        elif re.fullmatch(r"(down_blocks\.\d+|up_blocks\.\d+|mid_block)\.attentions\.\d+" + re.escape(PROCESSOR) + r"to_[kv]_ip\.weight", k):
            key = k
        else:
            raise ValueError("unexpected ip_adapter key %r" % (k,))
        if key in out:
            raise ValueError("ip_adapter key %r names the same weight as another key" % (k,))
        out[key] = v
    want = {b + PROCESSOR + n + ".weight" for b in block_prefixes(layers_per_block) for n in ("to_k_ip", "to_v_ip")}
    missing = sorted(want - set(out))
    if missing:
        raise ValueError("the adapter lacks %d of %d cross-attention weights, e.g. %s" % (len(missing), len(want), missing[0]))
    return out


def scale_list(scale, layers_per_block=2):
    """set_ip_adapter_scale's argument -> one float per transformer block in execution order.  A number: every block.  A dict {name: s} or a
    list of (name, s) pairs in the names `set_pag_applied_layers` takes ("down", "up.block_1", "mid", "down.block_0.attentions_1", ..):
    later entries override earlier ones, unnamed blocks get 0."""
    n = 6 * int(layers_per_block) + 4
    if isinstance(scale, bool):
        raise ValueError("the IP-Adapter scale has to be a number, a dict or a list of (name, scale) pairs but is %r" % (scale,))
    if isinstance(scale, (int, float)):
        out = [float(scale)] * n
    else:
        items = list(scale.items()) if hasattr(scale, "items") else list(scale)
        out = [0.0] * n
        for it in items:
            if not isinstance(it, (tuple, list)) or len(it) != 2:
                raise ValueError("the IP-Adapter scale list holds %r, expected (name, scale) pairs" % (it,))
            mask = pag_layer_mask(it[0], layers_per_block)
            for i in range(n):
                if (mask >> i) & 1:
                    out[i] = float(it[1])
    if not all(torch.isfinite(torch.tensor(out)).tolist()):
        raise ValueError("the IP-Adapter scales have to be finite but are %r" % (out,))
    return out


def split_embeds(embeds, negative=None, batch=None, do_cfg=True, seq=False):
    """the pipeline's `ip_adapter_image_embeds` / `negative_ip_adapter_image_embeds` -> (pos [B, E], neg [B, E] or None).  Takes [B, E],
    [B, 1, E], or diffusers' one-element list holding [2B, 1, E] (with CFG: the negatives first) or [B, 1, E].
    seq (a Plus adapter is loaded): the embeddings are hidden states, [B, T, E] or the list holding [2B, T, E] / [B, T, E], and come back
    as (pos [B, T, E], neg [B, T, E] or None)."""
    if isinstance(embeds, (list, tuple)):
        if len(embeds) != 1:
            raise ValueError("`ip_adapter_image_embeds` is a list of %d tensors: several adapters at once are not supported" % len(embeds))
        t = embeds[0]
        if batch is not None and do_cfg and t.shape[0] == 2 * batch:
            if negative is not None:
                raise ValueError("`ip_adapter_image_embeds` already holds the negatives ([2B, 1, E]); drop `negative_ip_adapter_image_embeds`")
            negative, t = t[:batch], t[batch:]
        embeds = t

    def flat(t, what):
        if seq:
            if t.dim() != 3 or t.shape[1] < 1:
                raise ValueError("%s has shape %s, expected [B, T, E]: the loaded adapter is a Plus adapter, which takes the image encoder's "
                                 "hidden states (hidden_states[-2]), not one embedding per image" % (what, tuple(t.shape)))
            if batch is not None and t.shape[0] != batch:
                raise ValueError("%s has batch %d, the prompt embeddings have %d" % (what, t.shape[0], batch))
            return t
        if t.dim() == 3 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 2:
            raise ValueError("%s has shape %s, expected [B, E] or [B, 1, E] (one embedding per image; token sequences go through the "
                             "UNet's ip_tokens=)" % (what, tuple(t.shape)))
        if batch is not None and t.shape[0] != batch:
            raise ValueError("%s has batch %d, the prompt embeddings have %d" % (what, t.shape[0], batch))
        return t
    pos = flat(embeds, "`ip_adapter_image_embeds`")
    neg = flat(negative, "`negative_ip_adapter_image_embeds`") if negative is not None else None
    if neg is not None and tuple(neg.shape) != tuple(pos.shape):
        raise ValueError("`negative_ip_adapter_image_embeds` has shape %s, the embeddings %s" % (tuple(neg.shape), tuple(pos.shape)))
    return pos, neg
