"""Test-local restatement of diffusers 0.14 UNet2DConditionModel.forward at ANY latent size, built from oracle.models' primitives.

oracle.models.unet_forward doubles every level on the up path (F.interpolate(scale_factor=2)), which is diffusers' arithmetic only when
both latent sides are multiples of 2**num_upsamplers = 8.  Otherwise diffusers sets `forward_upsample_size`: the stride-2 downsamplers
round a level UP (ceil(H / 2), as torch's conv does), and every Upsample2D stretches to the size of the skip it is concatenated with,
F.interpolate(size=skip.shape[2:], mode="nearest").  Everything else is oracle.models' code path unchanged."""
import math

import torch
import torch.nn.functional as F

from oracle import models as M


def nearest_src(d, n_in, n_out):
    """source index of output index d of F.interpolate(size=n_out, mode="nearest") over n_in pixels (aten nearest_idx, fp32 scale)"""
    if n_out == 2 * n_in:
        return d >> 1
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    return min(int(math.floor(float(torch.tensor(d, dtype=torch.float32) * scale))), n_in - 1)


def unet_forward(sd, cfg, sample, timestep, ehs, return_probe=False):
    boc = cfg["block_out_channels"]
    heads = cfg["num_heads"]
    L = cfg["layers_per_block"]
    G, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    n = sample.shape[0]
    forward_upsample_size = any(s % 8 != 0 for s in sample.shape[-2:])
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = M.conv(sd, "conv_in", sample)
    skips = [x]
    for i in range(4):
        for j in range(L):
            x = M.resnet(sd, "down_blocks.%d.resnets.%d" % (i, j), x, temb, G, eps)
            if i < 3:
                x = M.transformer2d(sd, "down_blocks.%d.attentions.%d" % (i, j), x, ehs, heads[i], G)
            skips.append(x)
        if i < 3:
            x = M.conv(sd, "down_blocks.%d.downsamplers.0.conv" % i, x, stride=2, padding=1)
            skips.append(x)
    x = M.resnet(sd, "mid_block.resnets.0", x, temb, G, eps)
    x = M.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads[3], G)
    x = M.resnet(sd, "mid_block.resnets.1", x, temb, G, eps)
    probe = x
    for i in range(4):
        for j in range(L + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = M.resnet(sd, "up_blocks.%d.resnets.%d" % (i, j), x, temb, G, eps)
            if i > 0:
                x = M.transformer2d(sd, "up_blocks.%d.attentions.%d" % (i, j), x, ehs, heads[3 - i], G)
        if i < 3:
            if forward_upsample_size:
                x = F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = M.conv(sd, "up_blocks.%d.upsamplers.0.conv" % i, x)
    x = M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G, eps)))
    return (x, probe) if return_probe else x
