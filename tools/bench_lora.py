"""LoRA on one GPU: what switching adapters costs, against what the project offered before (a host merge and a second UNet), and that the
forward itself does not change.

Full-size random-init UNet, one synthetic adapter per rank (--ranks, default 4 16 64 128) with a factor pair on EVERY conv and linear.

    set_adapters   (a) host wall time of unet.set_adapters([name]) including its one synchronisation, median of --rounds, and of the restore
                   set_adapters([]); (b) the same call between two events on its stream -- the span of the merge launches on the device --
                   with the weight bytes it moves (one read of the base copy, one write of the live weight; factors not counted) / time
    kernel         (b) ladi_op_lora_merge alone on three of the UNet's shapes (3x3 conv 1280 <- 1280, GEGLU 10240 <- 1280, linear 320 <- 320)
                   between events, --op-iters launches, bytes / time
    host_merge     (c) the route without this feature, once, at --host-rank: float32 torch merge of every weight on the host and a second
                   NativeUNet(cfg, merged) (skipped with --no-host)
    forward        (d) unet.time_forward(16, 64, 48) before any load / with an adapter active / after disable_lora(), interleaved rounds in
                   one process: the forward launches exactly what it launched before, so the three agree within run-to-run spread

Prints one JSON line.

    python tools/bench_lora.py [--ranks 4 16 64 128] [--rounds 3] [--forward-iters 10] [--op-iters 20] [--host-rank 16] [--no-host] [--size full]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pad64(c):
    return (c + 63) // 64 * 64


def make_adapter(shapes, rank, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m, s in shapes.items():
        sd[m + ".lora_down.weight"] = 0.05 * torch.randn((rank,) + tuple(s[1:]), generator=g)
        sd[m + ".lora_up.weight"] = 0.05 * torch.randn((s[0], rank), generator=g)
    return sd


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ranks", type=int, nargs="+", default=[4, 16, 64, 128])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--forward-iters", type=int, default=10)
    p.add_argument("--op-iters", type=int, default=20)
    p.add_argument("--host-rank", type=int, default=16)
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    a = p.parse_args()

    import ladi_vton_amd as L
    from ladi_vton_amd import _lib, configs as C
    from ladi_vton_amd._lib import stream_ptr
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cfg = C.UNET_FULL if a.size == "full" else C.UNET_TINY
    shapes = {k[:-len(".weight")]: s for k, s in C.unet_shapes(cfg).items() if k.endswith(".weight") and len(s) >= 2}
    taps = lambda s: s[2] * s[3] if len(s) == 4 else 1
    params = sum(s[0] * s[1] * taps(s) for s in shapes.values())
    weight_bytes = sum(2 * 2 * s[0] * taps(s) * pad64(s[1]) for s in shapes.values())       # base read + live write, fp16, padded rows
    res = {"metric": "lora_set_adapters_ms", "size": a.size, "device": torch.cuda.get_device_name(0), "targets": len(shapes), "params": params,
           "weight_bytes_moved": weight_bytes}

    t0 = time.perf_counter()
    unet = L.NativeUNet(cfg, C.synth_items(C.unet_shapes(cfg), "unet."))
    torch.cuda.synchronize()
    res["unet_create_s"] = time.perf_counter() - t0
    n, h, w, D = 16, 64, 48, cfg["cross_attention_dim"]
    ctx = torch.zeros((n, 77, D), dtype=torch.float16, device=dev)

    def forward_ms():
        unet.set_context(ctx)
        return unet.time_forward(n, h, w, a.forward_iters)

    forward_ms()                                                   # untimed: tile measurement, arena
    fw = {"before_load": [forward_ms() for _ in range(a.rounds)], "active": [], "disabled": []}

    # ---- (a), (b): switching adapters
    res["set_adapters"] = {}
    for rank in a.ranks:
        name = "r%d" % rank
        t0 = time.perf_counter()
        unet.load_lora_adapter(make_adapter(shapes, rank, rank), name)
        load_s = time.perf_counter() - t0
        wall, span, restore = [], [], []
        for r in range(a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            unet.set_adapters([name])
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            unet.set_adapters([])
            t3 = time.perf_counter()
            if r:
                wall.append((t1 - t0) * 1e3); span.append(e0.elapsed_time(e1)); restore.append((t3 - t2) * 1e3)
        sp = statistics.median(span)
        res["set_adapters"][name] = dict(load_s=load_s, wall_ms=statistics.median(wall), wall_ms_runs=wall, device_span_ms=sp, device_span_ms_runs=span,
                                         restore_wall_ms=statistics.median(restore), weight_tb_per_s=weight_bytes / (sp * 1e-3) / 1e12,
                                         fp32_tflops=2.0 * rank * params / (sp * 1e-3) / 1e12)

    # ---- (d): the forward, interleaved
    last = "r%d" % a.ranks[-1]
    for r in range(a.rounds):
        unet.set_adapters([last])
        fw["active"].append(forward_ms())
        unet.disable_lora()
        fw["disabled"].append(forward_ms())
    res["forward"] = dict(n=n, h=h, w=w, iters=a.forward_iters, adapter=last,
                          **{k + "_ms": statistics.median(v) for k, v in fw.items()}, **{k + "_ms_runs": v for k, v in fw.items()})

    # ---- (b): the kernel alone on three shapes of the UNet
    res["kernel"] = {}
    P = ctypes.c_void_p
    for label, (rows, cin, tp, half) in (("conv3x3_1280x1280", (1280, 1280, 9, 0)), ("geglu_10240x1280", (10240, 1280, 1, 5120)),
                                         ("linear_320x320", (320, 320, 1, 0))):
        cp = pad64(cin)
        base = torch.randn((rows, tp * cp), device=dev).half()
        live = torch.empty_like(base)
        for rank in a.ranks:
            up = (0.05 * torch.randn((rows, rank), device=dev)).contiguous()
            down = (0.05 * torch.randn((rank, tp, cin), device=dev)).contiguous()
            args = (base.data_ptr(), live.data_ptr(), tp * cp, cin, cp, tp, 0, rows, half, 1, (P * 8)(up.data_ptr()), (P * 8)(down.data_ptr()),
                    (ctypes.c_int * 8)(rank), (ctypes.c_float * 8)(1.0), None, stream_ptr())
            if lib.ladi_op_lora_merge(*args) != 0:
                raise RuntimeError(_lib.last_error())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.op_iters):
                lib.ladi_op_lora_merge(*args)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.op_iters
            byts = 2 * 2 * rows * tp * cp
            res["kernel"]["%s_r%d" % (label, rank)] = dict(us=ms * 1e3, weight_tb_per_s=byts / (ms * 1e-3) / 1e12,
                                                          fp32_tflops=2.0 * rank * rows * tp * cin / (ms * 1e-3) / 1e12)

    # ---- (c): the host route
    if not a.no_host:
        rank = a.host_rank
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        ad = make_adapter(shapes, rank, rank)
        base_sd = list(C.synth_items(C.unet_shapes(cfg), "unet."))          # the checkpoint a caller already holds: not timed
        t0 = time.perf_counter()
        merged = {}
        for k, v in base_sd:
            m = k[:-len(".weight")]
            if k.endswith(".weight") and m in shapes:
                d, u = ad[m + ".lora_down.weight"], ad[m + ".lora_up.weight"]
                v = v + (u @ d.reshape(rank, -1)).reshape(v.shape)
            merged[k] = v
        t1 = time.perf_counter()
        twin = L.NativeUNet(cfg, merged)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res["host_merge"] = dict(rank=rank, merge_s=t1 - t0, create_s=t2 - t1, total_s=t2 - t0)
        del twin, merged, base_sd
    print(json.dumps(res))


if __name__ == "__main__":
    main()
