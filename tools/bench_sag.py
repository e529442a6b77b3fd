"""Self-attention guidance (`sag_scale`) against the plain run, on one GPU: what the map capture and the second forward cost.

    kernels   sag_map (ladi_op_sag_map) on the mid block's Q / K shape of the CFG forward of B = 8 -- n = 16 samples, 20 heads, T = 48 at
              64x48 latents and T = 192 at 128x96 -- and sag_degrade (ladi_op_sag_degrade) on B = 8 at both latent sizes, wall time per
              call of the operator entries (each allocates its scratch and synchronises, so these are upper bounds of the launches)
    forward   the CFG forward of n = 16 at 64x48 and at 128x96 with the capture off and on, HIP events around NativeUNet.__call__, arms
              interleaved in one process on one UNet (--rounds after one untimed round); next to it two LayerNorm launches of the
              forward's largest shape (n * 3072 tokens of 320 channels), the yardstick the capture is held against
    call      512x384, B = 8, 50 DDIM steps, CFG 7.5 (BASELINE configs[1] shape): the fused run as bench.py runs it, one pipeline per arm,
              sag_scale 0 / 0.75 interleaved: --warmup untimed rounds, then --iters timed ones

Full-size random-init checkpoint and bench.py's synthetic rows.  Image quality on real weights is NOT evaluated here.  Prints one JSON line.

    python tools/bench_sag.py [--batch 8] [--rounds 3] [--forward-iters 10] [--iters 1] [--warmup 1] [--sag-scale 0.75] [--size full]
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

H, W, STEPS = 512, 384, 50


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--forward-iters", type=int, default=10)
    p.add_argument("--iters", type=int, default=1)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--sag-scale", type=float, default=0.75)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    p.add_argument("--skip-large", action="store_true", help="leave the 128x96 forward out")
    a = p.parse_args()

    import bench
    import ladi_vton_amd as L
    from ladi_vton_amd import _lib
    from ladi_vton_amd._lib import ptr, stream_ptr
    from oracle import configs as C
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg, vcfg = (C.UNET_FULL, C.VAE_FULL) if a.size == "full" else (C.UNET_TINY, C.VAE_TINY)
    ecfg = C.emasc_for_vae(vcfg)
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    lib = _lib.load()
    B, D, heads = a.batch, ucfg["cross_attention_dim"], ucfg["num_heads"][3]
    res = {"metric": "sag_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "sag_scale": a.sag_scale}
    sizes = [(64, 48)] + ([] if a.skip_large else [(128, 96)])
    g = torch.Generator().manual_seed(0)

    def wall_us(fn, iters=50):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    # ---- the kernels alone
    res["kernels"] = {}
    for h, w in sizes:
        hm, wm = unet.sag_tokens(h, w)
        T, n, Cc = hm * wm, 2 * B, heads * 64
        qkv = torch.randn((n * T, 3 * Cc), generator=g).to(dev, torch.float16)
        s = torch.empty((n, T), device=dev)
        m = torch.empty((n, T), dtype=torch.uint8, device=dev)
        k_ptr = ctypes.c_void_p(qkv.data_ptr() + 2 * Cc)
        us_map = wall_us(lambda: lib.ladi_op_sag_map(ptr(qkv), 3 * Cc, T * 3 * Cc, k_ptr, 3 * Cc, T * 3 * Cc, n, T, heads, ptr(s), ptr(m), stream_ptr()))
        lat = torch.randn((B, h * w, 4), generator=g).to(dev)
        eps = torch.randn((B, h * w, 4), generator=g).to(dev, torch.float16)
        rows = torch.zeros((2 * B * h * w, 64), dtype=torch.float16, device=dev)
        dst = ctypes.c_void_p(rows.data_ptr() + B * h * w * 64 * 2)
        mk = (torch.rand((B, hm, wm), generator=g) > 0.5).to(dev, torch.uint8)
        us_deg = wall_us(lambda: lib.ladi_op_sag_degrade(ptr(lat), ptr(eps), 4, ptr(mk), B, h, w, hm, wm, 0.8, 0.6, 1.0, ptr(rows), dst, 64, 64,
                                                         stream_ptr()))
        res["kernels"]["%dx%d" % (h, w)] = dict(T=T, n=n, heads=heads, sag_map_call_us=us_map, sag_degrade_call_us=us_deg)

    # ---- the forward with the capture off and on, and two LayerNorm launches of its largest shape
    res["forward"] = {}
    for h, w in sizes:
        ehs = torch.randn((2 * B, 77, D), generator=g).to(dev, torch.float16)
        x = (torch.randn((2 * B, ucfg["in_channels"], h, w), generator=g) * 0.5).to(dev, torch.float16)
        fw = {False: [], True: []}

        def forward_ms(on):
            unet.set_sag_capture(on)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            unet(x, 500, encoder_hidden_states=ehs)
            e0.record()
            for _ in range(a.forward_iters):
                unet(x, 500, encoder_hidden_states=ehs)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.forward_iters

        for r in range(a.rounds + 1):
            for on in (False, True):
                ms = forward_ms(on)
                if r:
                    fw[on].append(ms)
        unet.set_sag_capture(False)
        C0 = ucfg["block_out_channels"][0]
        rows_ln = 2 * B * h * w
        xl = torch.randn((rows_ln, C0), generator=g).to(dev, torch.float16)
        gam, bet, out = torch.ones(C0, device=dev, dtype=torch.float16), torch.zeros(C0, device=dev, dtype=torch.float16), torch.empty_like(xl)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ln = lambda: lib.ladi_op_layer_norm(ptr(xl), ptr(gam), ptr(bet), 1e-5, rows_ln, C0, ptr(out), stream_ptr())
        ln()
        e0.record()
        for _ in range(100):
            ln()
        e1.record()
        torch.cuda.synchronize()
        off, on_ = statistics.median(fw[False]), statistics.median(fw[True])
        res["forward"]["%dx%d" % (h, w)] = dict(n=2 * B, iters=a.forward_iters, off_ms=off, on_ms=on_, runs_off=fw[False], runs_on=fw[True],
                                                capture_us=(on_ - off) * 1e3, two_layer_norms_us=2 * e0.elapsed_time(e1) / 100 * 1e3)

    # ---- the whole call
    rows = bench.make_rows(0, B, H, W, 77, D, dev)
    call = {}
    for on in (False, True):
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
        call[on] = dict(pipe=pipe, loop_ms=[], seconds=[])
    for r in range(a.warmup + a.iters):
        for on in (False, True):
            arm = call[on]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arm["pipe"]._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                                   rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS,
                                   7.5, 1.0, False, True, return_device=True, out_uint8=True, sag_scale=a.sag_scale if on else 0.0)
            e1.record()
            torch.cuda.synchronize()
            if arm["pipe"].check_overflow():
                raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
            if r >= a.warmup:
                ms = (ctypes.c_float * 3)()
                if lib.ladi_tryon_stage_ms(arm["pipe"]._tryon, ms) != 0:
                    raise RuntimeError("no stage times")
                arm["loop_ms"].append(ms[1])
                arm["seconds"].append(e0.elapsed_time(e1) / 1e3)
    res["call"] = {"what": "%dx%d, %d DDIM steps, CFG 7.5" % (H, W, STEPS), "iters": a.iters, "warmup": a.warmup}
    for on, name in ((False, "off"), (True, "on")):
        arm = call[on]
        sec = statistics.median(arm["seconds"])
        res["call"][name] = dict(loop_ms=statistics.median(arm["loop_ms"]), loop_ms_runs=arm["loop_ms"], seconds=sec, seconds_runs=arm["seconds"],
                                 images_per_s=B / sec)
    res["call"]["loop_ratio"] = res["call"]["on"]["loop_ms"] / res["call"]["off"]["loop_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
