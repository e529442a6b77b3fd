"""IP-Adapter from a garment picture, on one GPU: what the once-per-call work between "a picture" and "image tokens" costs.

    encoder    CLIP ViT-H/14 (VISION_FULL, B pictures): ladi_vision_encoder_forward against ladi_vision_encoder_forward_ex with the
               penultimate output as well -- arms interleaved in one process on one encoder (--rounds after one untimed round), HIP events
    resampler  the Plus Resampler at the released sizes (E 1280, T 257, dim 1024, 16 heads of 64, depth 4, N 16, out 1024) alone, for
               n = B (the pictures) and n = 2B (the [neg ; pos] rows a CFG run hands to ladi_unet_set_ip_context_seq)
    call       512x384, B pictures, 50 DDIM steps, CFG 7.5 (BASELINE configs[1] shape), the fused run, three ways, one pipeline (one
               native handle, so its graphs stay captured) per arm, interleaved: plain; a Plus adapter with precomputed hidden states
               (`ip_adapter_image_embeds=`: the Resampler and the N = 16 image term); a Plus adapter with `ip_adapter_image=` (the
               pre-processing and the encoder forward on top: pipe.encode_image, then the same run).  Seconds per call from HIP events
               around the fused run, which hands back device uint8 images as bench.py's does

Full-size random-init weights everywhere; image quality is NOT evaluated here.  Prints one JSON line.

    python tools/bench_ip_image.py [--batch 8] [--rounds 3] [--iters 10] [--call-iters 1] [--warmup 1] [--size full|tiny]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, STEPS = 512, 384, 50


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--call-iters", type=int, default=1)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    a = p.parse_args()

    import bench
    import ladi_vton_amd as L
    from ladi_vton_amd import _lib
    from ladi_vton_amd._lib import check, ptr, stream_ptr
    from oracle import configs as C
    from tests import ip_image_ref as IR
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    full = a.size == "full"
    ucfg, vcfg, vis = (C.UNET_FULL, C.VAE_FULL, C.VISION_FULL) if full else (C.UNET_TINY, C.VAE_TINY, C.VISION_TINY)
    geo = dict(E=vis["hidden"], dim=1024, heads=16, depth=4, N=16) if full else dict(E=vis["hidden"], dim=128, heads=2, depth=2, N=16)
    ecfg = C.emasc_for_vae(vcfg)
    lib = _lib.load()
    B, D = a.batch, ucfg["cross_attention_dim"]
    res = {"metric": "ip_image_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "resampler_geometry": geo}

    # ---- the encoder
    enc = L.NativeCLIPVisionEncoder(vis, C.synth_items(C.vision_shapes(vis), "vision."))
    S, T, Hd = vis["image_size"], 1 + (vis["image_size"] // vis["patch_size"]) ** 2, vis["hidden"]
    px = torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(0)).to(dev, torch.float16)
    hid, pen = (torch.empty((B, T, Hd), dtype=torch.float16, device=dev) for _ in range(2))
    pooled = torch.empty((B, Hd), dtype=torch.float16, device=dev)
    arms = {
        "forward": lambda: check(lib.ladi_vision_encoder_forward(enc.h, ptr(px), 1, B, ptr(hid), ptr(pooled), stream_ptr()), "forward"),
        "forward_ex_with_penultimate": lambda: check(lib.ladi_vision_encoder_forward_ex(enc.h, ptr(px), 1, B, ptr(hid), ptr(pooled), ptr(pen), None,
                                                                                        stream_ptr()), "forward_ex"),
    }
    runs = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for k, fn in arms.items():
            ms = timed(fn, a.iters)
            if r:
                runs[k].append(ms)
    res["encoder"] = dict(tokens=T, iters=a.iters, runs=runs, **{k + "_ms": statistics.median(v) for k, v in runs.items()})

    # ---- the Resampler alone
    plus = IR.make_plus_adapter(ucfg, **geo)
    rs = L.NativeResampler(IR.resampler_of(plus), dim_head=geo["dim"] // geo["heads"])
    rruns = {}
    xs = {n: torch.randn((n, T, Hd), generator=torch.Generator().manual_seed(1)).to(dev, torch.float16) for n in (B, 2 * B)}
    outs = {n: torch.empty((n, geo["N"], D), dtype=torch.float16, device=dev) for n in xs}
    for r in range(a.rounds + 1):
        for n in xs:
            ms = timed(lambda: rs(xs[n], out=outs[n]), a.iters)
            if r:
                rruns.setdefault("n%d" % n, []).append(ms)
    res["resampler"] = dict(iters=a.iters, runs=rruns, **{k + "_ms": statistics.median(v) for k, v in rruns.items()})
    del rs

    # ---- the whole call
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    rows = bench.make_rows(0, B, H, W, 77, D, dev)
    picture = rows["cloth"]                                  # the in-shop garment picture, [B, 3, 512, 384] in [-1, 1]
    call = {}
    for name in ("plain", "plus_states", "plus_picture"):
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5], image_encoder=enc)
        call[name] = dict(pipe=pipe, seconds=[])
    unet.load_ip_adapter(plus, image_proj_dim_head=geo["dim"] // geo["heads"])
    cond, unc = call["plus_states"]["pipe"].encode_image(picture)
    cond, unc = cond.contiguous(), unc.contiguous()

    def ip_of(name, pipe):
        if name == "plain":
            return None
        if name == "plus_states":
            return cond, unc
        return tuple(t.contiguous() for t in pipe.encode_image(picture))      # what pipe(ip_adapter_image=) does before the fused run

    for r in range(a.warmup + a.call_iters):
        for name, arm in call.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arm["pipe"]._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                                   rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS,
                                   7.5, 1.0, False, True, return_device=True, out_uint8=True, ip=ip_of(name, arm["pipe"]))
            e1.record()
            torch.cuda.synchronize()
            if arm["pipe"].check_overflow():
                raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
            if r >= a.warmup:
                arm["seconds"].append(e0.elapsed_time(e1) / 1e3)
    res["call"] = {"what": "%dx%d, %d DDIM steps, CFG 7.5, B %d" % (H, W, STEPS, B), "iters": a.call_iters, "warmup": a.warmup}
    for name, arm in call.items():
        sec = statistics.median(arm["seconds"])
        res["call"][name] = dict(seconds=sec, seconds_runs=arm["seconds"], images_per_s=B / sec)
    res["call"]["plus_states_added_ms"] = 1e3 * (res["call"]["plus_states"]["seconds"] - res["call"]["plain"]["seconds"])
    res["call"]["plus_picture_added_ms"] = 1e3 * (res["call"]["plus_picture"]["seconds"] - res["call"]["plus_states"]["seconds"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
