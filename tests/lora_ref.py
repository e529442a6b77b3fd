"""Reference side of the LoRA tests: the float64 merge with its error bound, the packed-layout maps of the igemm weights, and a seeded
synthetic adapter maker.  Pure torch on the CPU; shared by tests/test_cpu_lora.py and tests/test_gpu_lora.py."""
from collections import OrderedDict

import numpy as np
import torch

from tests import util as U


def pad64(c):
    return (c + 63) // 64 * 64


def geglu_rows(half):
    """destination row of source row o of a GEGLU projection [2 half][cin] (load_geglu: blocks of 32 value rows | 32 gate rows)"""
    j = torch.arange(half)
    u = 64 * (j // 32) + j % 32
    return torch.cat([u, u + 32])


def row_map(rows, row0=0, geglu=False):
    """packed row of every source row of a target block: row0 + o, or row0 + the GEGLU interleave"""
    return row0 + (geglu_rows(rows // 2) if geglu else torch.arange(rows))


def pack_rows(w, total_rows=None, row0=0, geglu=False, fill=0.0):
    """diffusers [rows, cin] / [rows, cin, k, k] -> packed fp16 [total_rows, taps * cin_pad] (tap-major, channel-minor, channels zero-padded to a
    multiple of 64) with the block at its mapped rows; every other row holds `fill`"""
    rows, cin = w.shape[:2]
    taps = int(np.prod(w.shape[2:])) if w.dim() == 4 else 1
    cp = pad64(cin)
    total = rows if total_rows is None else total_rows
    out = torch.full((total, taps, cp), fill, dtype=torch.float16)
    blk = torch.zeros((rows, taps, cp), dtype=torch.float16)
    blk[:, :, :cin] = w.reshape(rows, cin, taps).permute(0, 2, 1).half()
    out[row_map(rows, row0, geglu)] = blk
    return out.reshape(total, taps * cp)


def unpack_rows(p, rows, cin, taps, row0=0, geglu=False):
    """the inverse of pack_rows for one block -> [rows, cin, taps] (float64)"""
    cp = pad64(cin)
    blk = p.reshape(p.shape[0], taps, cp)[row_map(rows, row0, geglu)]
    return blk[:, :, :cin].permute(0, 2, 1).double()


def fp32_scale(weight, alpha, rank):
    """the scale the library merges with: (float)((double)weight * alpha / rank)"""
    return float(np.float32(float(weight) * float(alpha) / float(rank)))


def merge_ref(base, factors):
    """float64 merge of one module.  base: [rows, cin] or [rows, cin, k, k]; factors: [(scale, up [rows, r], down [r, cin(, k, k)]), ..].
    Returns (ref, mag, K): ref = base + sum scale up @ down, mag = |base| + sum |scale| |up| @ |down| (what the bound scales with), K the
    summed rank, all in base's shape."""
    b = base.double()
    rows = b.shape[0]
    ref, mag, K = b.reshape(rows, -1).clone(), b.reshape(rows, -1).abs(), 0
    for scale, up, down in factors:
        up, down = up.double().reshape(rows, -1), down.double()
        d2 = down.reshape(down.shape[0], -1)
        ref = ref + float(scale) * (up @ d2)
        mag = mag + abs(float(scale)) * (up.abs() @ d2.abs())
        K += down.shape[0]
    return ref.reshape(b.shape), mag.reshape(b.shape), K


def merge_limit(ref, mag, K):
    """per-element limit of |got - ref| for the library's merge (tests/test_gpu_lora.py derives it):
        delta = (K + 4) 2^-24 mag,    limit = 1/2 ulp16(|ref| + delta) + delta"""
    delta = (K + 4) * U.U32 * mag
    return 0.5 * U.ulp16(ref.abs() + delta) + delta


def make_adapter(seed, shapes, ranks, amp=0.05, alpha=None, conv_up_4d=False):
    """seeded synthetic adapter in the library's own key form.  shapes: {module: weight shape} (diffusers), ranks: {module: rank}.
    Factors are amp * randn (float32); down keeps the conv's 4-D shape; alpha: None (no alpha keys: the rank), a number, or {module: number}.
    Returns an OrderedDict {<module>.lora_down.weight, <module>.lora_up.weight[, <module>.alpha]}."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for m, r in ranks.items():
        s = tuple(shapes[m])
        sd[m + ".lora_down.weight"] = amp * torch.randn((r,) + s[1:], generator=g)
        up = amp * torch.randn((s[0], r), generator=g)
        sd[m + ".lora_up.weight"] = up.reshape(s[0], r, 1, 1) if (conv_up_4d and len(s) == 4) else up
        a = alpha.get(m) if isinstance(alpha, dict) else alpha
        if a is not None:
            sd[m + ".alpha"] = torch.tensor(float(a))
    return sd


def adapter_factors(sd, module):
    """(down, up [rows, r], alpha) of one module of a make_adapter dict"""
    down, up = sd[module + ".lora_down.weight"], sd[module + ".lora_up.weight"]
    up = up.reshape(up.shape[0], up.shape[1])
    alpha = float(sd[module + ".alpha"]) if module + ".alpha" in sd else float(down.shape[0])
    return down, up, alpha


def merged_state_dict(base_sd, active):
    """float64 reference of set_adapters: active = [(adapter dict, weight), ..] in merge order.  Returns {key: (ref, mag, K)} for every
    `.weight` key some adapter touches"""
    out = OrderedDict()
    mods = []
    for sd, _ in active:
        for k in sd:
            if k.endswith(".lora_down.weight") and k[:-len(".lora_down.weight")] not in mods:
                mods.append(k[:-len(".lora_down.weight")])
    for m in mods:
        fs = []
        for sd, w in active:
            if m + ".lora_down.weight" in sd:
                down, up, alpha = adapter_factors(sd, m)
                fs.append((fp32_scale(w, alpha, down.shape[0]), up, down))
        out[m + ".weight"] = merge_ref(base_sd[m + ".weight"], fs)
    return out
