"""fp16 headroom probe: per-layer activation magnitudes and non-finite counts of the native UNet / VAE / EMASC (ladi_probe_*).

All activations are stored in fp16 (largest finite value 65504).  A RangeProbe attached to modules records, for every named activation
(diffusers key prefix of the producing module, include/ladi_native.h), the largest finite |x| and how many elements were inf / NaN,
so a checkpoint that leaves the fp16 range is reported by layer instead of ending in NaN latents and a grey image.  Opt-in: without a
probe the modules launch exactly what they launched before.
"""
from ctypes import c_float, c_uint

from . import _lib
from ._lib import NativeError, check, stream_ptr

FP16_MAX = 65504.0


def unet_point_names(cfg):
    """probe points of one UNet forward, in execution order"""
    L = cfg["layers_per_block"]
    n = ["conv_in"]
    for i in range(4):
        for j in range(L):
            n.append("down_blocks.%d.resnets.%d" % (i, j))
            if i < 3:
                n.append("down_blocks.%d.attentions.%d" % (i, j))
        if i < 3:
            n.append("down_blocks.%d.downsamplers.0" % i)
    n += ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
    for i in range(4):
        for j in range(L + 1):
            n.append("up_blocks.%d.resnets.%d" % (i, j))
            if i > 0:
                n.append("up_blocks.%d.attentions.%d" % (i, j))
        if i < 3:
            n.append("up_blocks.%d.upsamplers.0" % i)
    return n + ["conv_out"]


def vae_encoder_point_names():
    return ["encoder.conv_in"] + ["encoder.down_blocks.%d" % i for i in range(4)] + ["encoder.mid_block", "quant_conv"]


def vae_decoder_point_names():
    return ["post_quant_conv", "decoder.mid_block"] + ["decoder.up_blocks.%d" % i for i in range(4)] + ["decoder.conv_out"]


def emasc_point_names(cfg):
    return ["emasc.%d" % i for i in range(len(cfg["in_channels"]))]


class RangeProbe:
    """probe = RangeProbe(); probe.attach(unet, vae, emasc); ...run...; probe.report() -> [(name, absmax, absmax / 65504, nonfinite)]
    in execution order.  Values accumulate (max / sum) over every run until reset()."""

    def __init__(self, max_points=512):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.h = self.lib.ladi_probe_create(int(max_points))
        if not self.h:
            raise NativeError("ladi_probe_create failed: " + _lib.last_error())
        self.max_points = int(max_points)
        self.raise_on_nonfinite = False
        self._attached = []

    @staticmethod
    def _attach_fn(lib, m):
        from .modules import NativeEMASC, NativeUNet, NativeVAE
        for cls, fn in ((NativeUNet, lib.ladi_unet_attach_probe), (NativeVAE, lib.ladi_vae_attach_probe), (NativeEMASC, lib.ladi_emasc_attach_probe)):
            if isinstance(m, cls):
                return fn
        raise TypeError("RangeProbe.attach: expected NativeUNet / NativeVAE / NativeEMASC, got %r" % type(m).__name__)

    def attach(self, *modules):
        for m in modules:
            if m is None or any(a is m for a in self._attached):
                continue
            check(self._attach_fn(self.lib, m)(m.h, self.h), "ladi_*_attach_probe")
            self._attached.append(m)
        return self

    def detach(self, *modules):
        """detach from these modules; with none given, from every module"""
        held = getattr(self, "_attached", [])
        gone = [m for m in held if not modules or any(m is x for x in modules)]
        for m in gone:
            if getattr(m, "h", None):
                self._attach_fn(self.lib, m)(m.h, None)
        self._attached = [m for m in held if not any(m is g for g in gone)]

    def attach_only(self, *modules):
        """attach to exactly these modules (None entries are skipped): whatever was attached and is not among them is detached"""
        keep = [m for m in modules if m is not None]
        stale = [m for m in self._attached if not any(m is k for k in keep)]
        if stale:
            self.detach(*stale)
        return self.attach(*keep)

    def reset(self):
        check(self.lib.ladi_probe_reset(self.h, stream_ptr()), "ladi_probe_reset")

    def names(self):
        return [self.lib.ladi_probe_name(self.h, i).decode() for i in range(self.lib.ladi_probe_count(self.h))]

    def _read(self):
        """-> (names, absmax list, nonfinite list, rank list); waits for the current stream.  rank: the order in time (1, 2, ...) in which
        the points first held an inf / NaN, 0 = never"""
        n = self.lib.ladi_probe_count(self.h)
        am, nf, rk = (c_float * max(n, 1))(), (c_uint * max(n, 1))(), (c_uint * max(n, 1))()
        rc = self.lib.ladi_probe_read(self.h, am, nf, n, stream_ptr())
        if rc >= 0:
            rc = self.lib.ladi_probe_read_rank(self.h, rk, n, stream_ptr())
        if rc < 0:
            raise NativeError("ladi_probe_read failed (rc=%d): %s" % (rc, _lib.last_error()))
        return self.names()[:n], list(am)[:n], list(nf)[:n], list(rk)[:n]

    def report(self):
        """[(name, absmax, absmax / 65504, nonfinite)] in execution order; absmax is over the finite elements, at the tensor's true scale"""
        names, am, nf, _ = self._read()
        return [(k, float(a), float(a) / FP16_MAX, int(c)) for k, a, c in zip(names, am, nf)]

    def first_nonfinite(self):
        """name of the point that held an inf / NaN FIRST IN TIME, or None.  For one forward that is the first such point in execution
        order; over a denoising loop the NaNs of one evaluation come back into conv_in at the next, and the layer that started it is the
        one reported"""
        names, _, nf, rank = self._read()
        hit = [(r, i) for i, (r, c) in enumerate(zip(rank, nf)) if c and r]
        return names[min(hit)[1]] if hit else None

    @staticmethod
    def format(report, sort_by_headroom=True):
        """the report as a text table; sort_by_headroom: least head-room (largest absmax, non-finite first) on top"""
        rows = sorted(report, key=lambda r: (-min(r[3], 1), -r[1])) if sort_by_headroom else list(report)
        w = max([len(r[0]) for r in rows] + [5])
        out = ["%-*s  %12s  %9s  %10s" % (w, "point", "absmax", "of 65504", "nonfinite")]
        for name, a, frac, cnt in rows:
            out.append("%-*s  %12.5g  %8.4f%%  %10d" % (w, name, a, 100.0 * frac, cnt))
        return "\n".join(out)

    def __del__(self):
        try:
            self.detach()
        finally:
            if getattr(self, "h", None):
                self.lib.ladi_probe_destroy(self.h)
                self.h = None
