"""fp32 reference of the UNet range-probe points: tests/ref_unet.py's forward (oracle.models' block functions in the oracle's order), which
hands every tensor a probe point names to an observer; here the observer records max |x|."""
from collections import OrderedDict

from tests import ref_unet as RU


def unet_point_absmax(sd, cfg, sample, timestep, ehs):
    """-> (OrderedDict name -> fp32 max |x| in probe-point order, the forward's output)"""
    out = OrderedDict()
    x = RU.unet_forward(sd, cfg, sample, timestep, ehs, observe=lambda name, t: out.__setitem__(name, float(t.abs().max())))
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
