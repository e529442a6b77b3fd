"""The IP-Adapter image term against the plain UNet forward, on one GPU.

    forward   the CFG forward of B = 8 (n = 16 samples of 64x48 latents, 77 text tokens) timed with unet.time_forward, arms interleaved in
              one process on one UNet (--rounds rounds after one untimed round), for N = 4 and N = 16 image tokens:
                (a) plain: no image context            (b) image term by csrc/ip_adapter.hip (route 0, shipped)
                (c) image term by the kernels that existed before: flash_attn64 over the N keys into scratch + a scaled add (route 1)
    kernel    (d) ip_attn_add alone at the four shapes a forward runs it at, against its byte count 3 * n T C * 2 (q read, o read, o
              written), and flash_attn64 over the same N keys alone (the first half of route 1: a lower bound of what (c) costs there).
              Each timed launch works on another q / o pair of a pool larger than the 256 MiB Infinity Cache.

Full-size random-init checkpoint, a random adapter with E = 1024.  Image quality on real weights is NOT evaluated here.  Prints one JSON
line.  The count of launches the image term adds is the definition (one per transformer block: 16; route 1: 32), not a device count.

    python tools/bench_ip_adapter.py [--batch 8] [--rounds 3] [--forward-iters 10] [--kernel-iters 200] [--size full|tiny]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 512, 384
HBM_TBS = 6.29          # what a streaming copy reaches on MI355X (8.0 TB/s spec)


def kernel_arm(lib, n, T, heads, N, iters, dev):
    """-> dict(us, gb_s, flash_us) of one level's shape"""
    from ladi_vton_amd._lib import ptr, stream_ptr
    Cc = heads * 64
    set_bytes = 2 * n * T * Cc * 2
    sets = max(2, min(96, -(-(320 << 20) // set_bytes)))
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn((sets, n, T, Cc), generator=g, device=dev, dtype=torch.float16)
    o = torch.randn((sets, n, T, Cc), generator=g, device=dev, dtype=torch.float16)
    kv = torch.randn((n, N, 2 * Cc), generator=g, device=dev, dtype=torch.float16)
    vptr = ctypes.c_void_p(kv.data_ptr() + Cc * 2)

    def ip(i):
        rc = lib.ladi_op_ip_attn_add(ptr(q[i]), Cc, T * Cc, ptr(kv), 2 * Cc, N * 2 * Cc, vptr, 2 * Cc, N * 2 * Cc, ptr(o[i]), Cc, T * Cc, n, heads, T, N,
                                     1e-3, stream_ptr())
        assert rc == 0, rc

    def flash(i):
        rc = lib.ladi_op_attention(ptr(q[i]), ptr(kv), vptr, ptr(o[i]), Cc, 2 * Cc, 2 * Cc, Cc, T * Cc, N * 2 * Cc, N * 2 * Cc, T * Cc, n, heads, T, N,
                                   0.125, stream_ptr())
        assert rc == 0, rc
    out = {}
    for name, fn in (("ip", ip), ("flash", flash), ("ip", ip), ("flash", flash)):          # interleaved, two windows each
        for i in range(min(sets, 8)):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % sets)
        e1.record()
        torch.cuda.synchronize()
        out.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3 / iters)
    us = min(out["ip"])
    moved = 3 * n * T * Cc * 2
    return dict(n=n, T=T, heads=heads, N=N, sets=sets, us=us, us_runs=out["ip"], bytes=moved, gb_s=moved / us / 1e3,
                bound_us=moved / (HBM_TBS * 1e6), flash_us=min(out["flash"]), flash_us_runs=out["flash"])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--forward-iters", type=int, default=10)
    p.add_argument("--kernel-iters", type=int, default=200)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    a = p.parse_args()

    import ladi_vton_amd as L
    from ladi_vton_amd import _lib
    from ladi_vton_amd._lib import check
    from oracle import configs as C
    from tests import ip_adapter_ref as R
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg = C.UNET_FULL if a.size == "full" else C.UNET_TINY
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    lib = _lib.load()
    B, D, E = a.batch, ucfg["cross_attention_dim"], 1024
    n, h, w = 2 * B, H // 8, W // 8
    res = {"metric": "ip_adapter_forward_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "launches_added": 16,
           "launches_added_route1": 32, "forward": {}, "kernel": []}
    unet.set_context(torch.zeros((n, 77, D), dtype=torch.float16, device=dev))
    emb = torch.randn((n, E), generator=torch.Generator().manual_seed(3)).half().to(dev)
    for N in (4, 16):
        unet.load_ip_adapter(R.make_adapter(ucfg, N, E))
        fw = {"plain": [], "ip": [], "flash_add": []}
        for r in range(a.rounds + 1):
            for arm in ("plain", "ip", "flash_add"):
                unet.set_ip_context(None if arm == "plain" else emb)
                check(lib.ladi_unet_set_ip_route(unet.h, 1 if arm == "flash_add" else 0), "ladi_unet_set_ip_route")
                ms = unet.time_forward(n, h, w, a.forward_iters)
                if r:
                    fw[arm].append(ms)
        check(lib.ladi_unet_set_ip_route(unet.h, 0), "ladi_unet_set_ip_route")
        unet.set_ip_context(None)
        unet.unload_ip_adapter()
        med = {k: statistics.median(v) for k, v in fw.items()}
        res["forward"]["N%d" % N] = dict(n=n, h=h, w=w, iters=a.forward_iters, plain_ms=med["plain"], ip_ms=med["ip"], flash_add_ms=med["flash_add"],
                                         runs=fw, ip_added_ms=med["ip"] - med["plain"], ip_added_pct=100.0 * (med["ip"] - med["plain"]) / med["plain"],
                                         flash_add_added_ms=med["flash_add"] - med["plain"])
    heads, hw = ucfg["num_heads"], h * w
    for N in (4, 16):
        for lvl, (T, hd) in enumerate(((hw, heads[0]), (hw // 4, heads[1]), (hw // 16, heads[2]), (hw // 64, heads[3]))):
            k = kernel_arm(lib, n, T, hd, N, a.kernel_iters, dev)
            k["level"] = lvl
            res["kernel"].append(k)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
