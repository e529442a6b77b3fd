"""The one reference UNet forward the test oracles share: diffusers 0.14 UNet2DConditionModel.forward composed from oracle.models' block
functions, at ANY latent size, with every optional term the library has.  Each feature's own mathematics stays in its module
(tests/freeu_ref.py, tests/tome_ref.py, ..); this module only says where in the walk it acts.  With every option at its off value the
forward is oracle.models.unet_forward bit for bit at latent sizes that are multiples of 8 (tests/test_cpu_anysize.py and the features'
CPU tests assert it).  Nothing here imports the package under test.

    any size    oracle.models.unet_forward doubles every level on the up path (F.interpolate(scale_factor=2)), which is diffusers' arithmetic
                only when both latent sides are multiples of 2**num_upsamplers = 8.  Otherwise diffusers sets `forward_upsample_size`: the
                stride-2 downsamplers round a level UP (ceil(H / 2), as torch's conv does), and every Upsample2D stretches to the size of the
                skip it is concatenated with, F.interpolate(size=skip.shape[2:], mode="nearest")
    freeu       None or (s1, s2, b1, b2): freeu_ref.apply_freeu before every concatenation of up_blocks.0 and up_blocks.1
    cache       None, ("capture", k) or ("shallow", k, tensor), L = layers_per_block, 0 <= k <= L.  Capture: the whole forward, which also
                hands back the hidden state that enters up_blocks.3.resnets.(L - k), before the concatenation with its skip (the output of
                up_blocks.3.attentions.(L - k - 1) for k < L, of up_blocks.2.upsamplers.0 for k = L) -> (out, captured).  Shallow: conv_in,
                layers 0 .. k-1 of down_blocks.0, then up_blocks.3 layers L-k .. L, the first from the tensor, conv_norm_out, conv_out;
                the time embedding of the evaluation's own timestep.  It runs neither FreeU stage
    pag         None or (layer prefixes, pag_first): identity self-attention (O = V) for the samples [pag_first, n) in those blocks;
                pag_first None or >= n: none
    ip          None or (sd_ip, tokens [n, N, cross_dim], scales): one scale per transformer block in execution order (block_prefixes);
                a block whose scale is 0 has no image term
    tome        None or (tcfg, forced, record, metric): token merging in the blocks of the first max_downsample levels; forced: None or a
                dict prefix -> a plan per sample; record(p, t0, plans): a hook; metric: "proj_in" (the contract) or a mis-wiring
    observe     None or observe(name, x), called with the output of every range-probe point: "conv_in", every resnet's and transformer's
                prefix, "down_blocks.i.downsamplers.0", "up_blocks.i.upsamplers.0" (after its conv), "conv_out"
"""
import math

import torch
import torch.nn.functional as F

from oracle import models as M
from tests import freeu_ref as FU
from tests import tome_ref as TM


def nearest_src(d, n_in, n_out):
    """source index of output index d of F.interpolate(size=n_out, mode="nearest") over n_in pixels (aten nearest_idx, fp32 scale)"""
    if n_out == 2 * n_in:
        return d >> 1
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    return min(int(math.floor(float(torch.tensor(d, dtype=torch.float32) * scale))), n_in - 1)


def block_prefixes(L=2):
    """the transformer blocks in execution order: bit i of the library's PAG mask, entry i of the IP scales, is entry i"""
    return (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] + ["mid_block.attentions.0"] +
            ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)])


def level_of(prefix, L=2):
    """resolution level of a transformer block by its diffusers prefix: down_blocks.i -> i, mid -> 3, up_blocks.i -> 3 - i"""
    p = prefix.split(".")
    return 3 if p[0] == "mid_block" else int(p[1]) if p[0] == "down_blocks" else 3 - int(p[1])


def merged_prefixes(tcfg, L=2):
    """the blocks a token-merging configuration merges, in execution order (the order of the library's merged-block index)"""
    return [p for p in block_prefixes(L) if level_of(p, L) < tcfg["max_downsample"]]


def transformer2d(sd, p, x, ehs, heads, groups, *, perturbed_from=None, ip=None, tome=None):
    """oracle.models.transformer2d's sequence with three optional terms.  perturbed_from: attention(q, k, v) swapped for v in attn1 on the
    samples [perturbed_from, n).  ip = (sd_ip, tokens, scale of THIS block): scale * attention(q2, to_k_ip(tokens), to_v_ip(tokens)) added
    to the attn2 output before to_out, q2 from the merged rows when merge_crossattn is on.  tome = (tcfg, forced, record, metric): tcfg the
    configuration dict; forced: a plan per sample (else the plan is computed here, in x's dtype, from the output of proj_in); record(p, t0,
    plans): a hook; metric: "proj_in", or a mis-wiring "norm1" / "input" the wiring test measures against."""
    n, C, h, w = x.shape
    res = x
    g = M.group_norm(sd, p + ".norm", x, groups, 1e-6).permute(0, 2, 3, 1).reshape(n, h * w, C)
    t = M.linear(sd, p + ".proj_in", g)
    b = p + ".transformer_blocks.0"
    k0 = n if perturbed_from is None else max(0, min(n, perturbed_from))
    tcfg, plans = None, None
    if tome is not None:
        tcfg, forced, record, metric = tome
        sp, dp = TM.tables(h, w, 2, 2, tcfg["use_rand"], tcfg["seed"])
        r = TM.merge_count(h * w, len(sp), tcfg["ratio"]) if dp else 0
        if r > 0:
            assert k0 == n, "the library refuses a block that both merges tokens and is perturbed: " + p
            if forced is not None:
                plans = forced
            else:
                met = {"proj_in": t, "norm1": M.layer_norm(sd, b + ".norm1", t), "input": g}[metric]
                plans = [TM.plan_of_metric(met[s], sp, dp, r, x.dtype) for s in range(n)]
            if record is not None:
                record(p, t, plans)
    m = (lambda a: torch.stack([TM.merge(a[s], plans[s], a.dtype) for s in range(n)]))
    u = (lambda y: torch.stack([TM.unmerge(y[s], plans[s]) for s in range(n)]))
    on = lambda flag: plans is not None and tcfg[flag]

    a = M.layer_norm(sd, b + ".norm1", t)
    a = m(a) if on("merge_attn") else a
    q, k, v = M.linear(sd, b + ".attn1.to_q", a), M.linear(sd, b + ".attn1.to_k", a), M.linear(sd, b + ".attn1.to_v", a)
    if k0 == n:
        o = M.attention(q, k, v, heads)
    else:
        o = v.clone()                                     # the identity attention map: O = V
        if k0 > 0:
            o[:k0] = M.attention(q[:k0], k[:k0], v[:k0], heads)
    o = M.linear(sd, b + ".attn1.to_out.0", o)
    t = (u(o) if on("merge_attn") else o) + t
    a = M.layer_norm(sd, b + ".norm2", t)
    a = m(a) if on("merge_crossattn") else a
    q2 = M.linear(sd, b + ".attn2.to_q", a)
    o = M.attention(q2, M.linear(sd, b + ".attn2.to_k", ehs), M.linear(sd, b + ".attn2.to_v", ehs), heads)
    if ip is not None and float(ip[2]) != 0.0:
        sd_ip, tokens, scale = ip
        o = o + float(scale) * M.attention(q2, F.linear(tokens, sd_ip[b + ".attn2.processor.to_k_ip.weight"]),
                                           F.linear(tokens, sd_ip[b + ".attn2.processor.to_v_ip.weight"]), heads)
    o = M.linear(sd, b + ".attn2.to_out.0", o)
    t = (u(o) if on("merge_crossattn") else o) + t
    a = M.layer_norm(sd, b + ".norm3", t)
    a = m(a) if on("merge_mlp") else a
    uu, gg = M.linear(sd, b + ".ff.net.0.proj", a).chunk(2, dim=-1)
    o = M.linear(sd, b + ".ff.net.2", uu * F.gelu(gg))
    t = (u(o) if on("merge_mlp") else o) + t
    t = M.linear(sd, p + ".proj_out", t)
    return t.reshape(n, h, w, C).permute(0, 3, 1, 2) + res


def unet_forward(sd, cfg, sample, timestep, ehs, *, freeu=None, cache=None, pag=None, ip=None, tome=None, observe=None):
    """-> out, or (out, captured) with cache = ("capture", k).  One loop body for the whole and the shallow forward: a layer either runs
    or is skipped."""
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G_, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    n = sample.shape[0]
    mode, k = (None, 0) if cache is None else (cache[0], int(cache[1]))
    assert mode in (None, "capture", "shallow") and 0 <= k <= L
    shallow = mode == "shallow"
    layers, pag_first = (set(), None) if pag is None else (set(pag[0]), pag[1])
    assert not (shallow and layers and pag_first is not None and pag_first < n), "the library refuses pag_first with a feature cache"
    index = {b: i for i, b in enumerate(block_prefixes(L))}
    if ip is not None:
        assert len(ip[2]) == len(index) and ip[1].shape[0] == n

    def see(name, x):
        if observe is not None:
            observe(name, x)
        return x

    def res(p, x):
        return see(p, M.resnet(sd, p, x, temb, G_, eps))

    def xf(p, x, hd):
        merges = tome is not None and tome[0] is not None and tome[0]["ratio"] > 0 and p in merged_prefixes(tome[0], L)
        tm = (tome[0], tome[1].get(p) if tome[1] else None, tome[2], tome[3]) if merges else None
        return see(p, transformer2d(sd, p, x, ehs, hd, G_, perturbed_from=pag_first if p in layers else None,
                                    ip=None if ip is None else (ip[0], ip[1], ip[2][index[p]]), tome=tm))
    forward_upsample_size = any(s % 8 != 0 for s in sample.shape[-2:])
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = see("conv_in", M.conv(sd, "conv_in", sample))
    skips = [x]
    for i in range(4):
        for j in range(L):
            if shallow and (i > 0 or j >= k):
                continue
            x = res("down_blocks.%d.resnets.%d" % (i, j), x)
            if i < 3:
                x = xf("down_blocks.%d.attentions.%d" % (i, j), x, heads[i])
            skips.append(x)
        if i < 3 and not shallow:
            x = see("down_blocks.%d.downsamplers.0" % i, M.conv(sd, "down_blocks.%d.downsamplers.0.conv" % i, x, stride=2, padding=1))
            skips.append(x)
    if not shallow:
        x = res("mid_block.resnets.0", x)
        x = xf("mid_block.attentions.0", x, heads[3])
        x = res("mid_block.resnets.1", x)
    captured = None
    for i in range(4):
        for j in range(L + 1):
            cache_pt = i == 3 and j == L - k
            if shallow and not cache_pt and (i < 3 or j < L - k):
                continue
            if cache_pt and shallow:
                assert cache[2].shape == (n, boc[1 if k == L else 0]) + tuple(sample.shape[-2:]), (cache[2].shape, sample.shape)
                x = cache[2]
            elif cache_pt and mode == "capture":
                captured = x.clone()
            x, sk = FU.apply_freeu(i, x, skips.pop(), freeu)
            x = torch.cat([x, sk], dim=1)
            x = res("up_blocks.%d.resnets.%d" % (i, j), x)
            if i > 0:
                x = xf("up_blocks.%d.attentions.%d" % (i, j), x, heads[3 - i])
        if i < 3 and not shallow:
            if forward_upsample_size:
                x = F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = see("up_blocks.%d.upsamplers.0" % i, M.conv(sd, "up_blocks.%d.upsamplers.0.conv" % i, x))
    assert not skips
    x = see("conv_out", M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G_, eps))))
    return (x, captured) if mode == "capture" else x
