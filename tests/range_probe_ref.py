"""fp32 reference of the UNet range-probe points: the block sequence of oracle.models.unet_forward re-run from the oracle's public
functions (conv, resnet, transformer2d; same order), recording max |x| of every tensor a probe point names."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import models as M


def unet_point_absmax(sd, cfg, sample, timestep, ehs):
    """-> (OrderedDict name -> fp32 max |x| in probe-point order, the forward's output)"""
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    out = OrderedDict()

    def rec(name, x):
        out[name] = float(x.abs().max())
        return x

    n = sample.shape[0]
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = rec("conv_in", M.conv(sd, "conv_in", sample))
    skips = [x]
    for i in range(4):
        for j in range(L):
            p = "down_blocks.%d.resnets.%d" % (i, j)
            x = rec(p, M.resnet(sd, p, x, temb, G, eps))
            if i < 3:
                p = "down_blocks.%d.attentions.%d" % (i, j)
                x = rec(p, M.transformer2d(sd, p, x, ehs, heads[i], G))
            skips.append(x)
        if i < 3:
            p = "down_blocks.%d.downsamplers.0" % i
            x = rec(p, M.conv(sd, p + ".conv", x, stride=2, padding=1))
            skips.append(x)
    x = rec("mid_block.resnets.0", M.resnet(sd, "mid_block.resnets.0", x, temb, G, eps))
    x = rec("mid_block.attentions.0", M.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads[3], G))
    x = rec("mid_block.resnets.1", M.resnet(sd, "mid_block.resnets.1", x, temb, G, eps))
    for i in range(4):
        for j in range(L + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            p = "up_blocks.%d.resnets.%d" % (i, j)
            x = rec(p, M.resnet(sd, p, x, temb, G, eps))
            if i > 0:
                p = "up_blocks.%d.attentions.%d" % (i, j)
                x = rec(p, M.transformer2d(sd, p, x, ehs, heads[3 - i], G))
        if i < 3:
            p = "up_blocks.%d.upsamplers.0" % i
            x = rec(p, M.conv(sd, p + ".conv", F.interpolate(x, scale_factor=2.0, mode="nearest")))
    x = rec("conv_out", M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G, eps))))
    return out, x


def scaled_checkpoint(sd, prefix, factor):
    """copy of sd with `prefix`.weight / .bias multiplied by factor (a power of two: exact)"""
    sd2 = dict(sd)
    for k in (prefix + ".weight", prefix + ".bias"):
        sd2[k] = sd[k] * factor
    return sd2


def overflow_exponent(sd, cfg, sample, timestep, ehs, prefix, point, target=4 * 65504.0):
    """smallest k >= 1 (searched upwards from the ratio of the unscaled magnitude) such that, with `prefix` scaled by 2^k, the fp32
    max |x| at `point` exceeds target; -> (k, that max)"""
    import math
    base = unet_point_absmax(sd, cfg, sample, timestep, ehs)[0][point]
    k = max(1, int(math.ceil(math.log2(target / base))))
    while True:
        got = unet_point_absmax(scaled_checkpoint(sd, prefix, 2.0 ** k), cfg, sample, timestep, ehs)[0][point]
        if got > target:
            return k, got
        k += 1
