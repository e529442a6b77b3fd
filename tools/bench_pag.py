"""Perturbed-attention guidance (`pag_scale`) against the plain run, on one GPU: what the third sample group costs.

    forward   the CFG forward of B = 8 at 64x48: n = 16 samples (no perturbed group) against n = 24 with the last 8 perturbed, for the
              default layer ("mid") and for all sixteen blocks, timed with HIP events around NativeUNet.__call__(pag_first=) -- the same
              entry (ladi_unet_forward_pag) for every arm, arms interleaved in one process on one UNet (--rounds after one untimed round)
    call      512x384, B = 8, 50 DDIM steps, CFG 7.5 (BASELINE configs[1] shape): the fused run as bench.py runs it, one pipeline (one
              native handle, so its graphs stay captured) per arm, PAG off / on (pag_scale 3.0, default layer) interleaved: --warmup
              untimed rounds, then --iters timed ones

Full-size random-init checkpoint and bench.py's synthetic rows.  Image quality on real weights is NOT evaluated here: the checkpoint is
random-init.  Prints one JSON line.

    python tools/bench_pag.py [--batch 8] [--rounds 3] [--forward-iters 10] [--iters 1] [--warmup 1] [--pag-scale 3.0]
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

H, W, STEPS = 512, 384, 50


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--forward-iters", type=int, default=10)
    p.add_argument("--iters", type=int, default=1)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--pag-scale", type=float, default=3.0)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    a = p.parse_args()

    import bench
    import ladi_vton_amd as L
    from ladi_vton_amd import _lib
    from oracle import configs as C
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg, vcfg = (C.UNET_FULL, C.VAE_FULL) if a.size == "full" else (C.UNET_TINY, C.VAE_TINY)
    ecfg = C.emasc_for_vae(vcfg)
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    lib = _lib.load()
    B, D = a.batch, ucfg["cross_attention_dim"]
    res = {"metric": "pag_forward_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "pag_scale": a.pag_scale}

    # ---- the forward alone: one context of 3B samples, every arm runs its leading rows of it
    h, w = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    ehs = torch.randn((3 * B, 77, D), generator=g).to(dev, torch.float16)
    x = (torch.randn((3 * B, ucfg["in_channels"], h, w), generator=g) * 0.5).to(dev, torch.float16)
    arms = {"n16": (2 * B, "mid"), "n24_mid": (3 * B, "mid"), "n24_all": (3 * B, ["down", "mid", "up"])}
    fw = {k: [] for k in arms}

    def forward_ms(n, layers):
        unet.set_pag_applied_layers(layers)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        unet(x[:n], 500, encoder_hidden_states=ehs, pag_first=2 * B)        # planning pass and tile selection of this shape
        e0.record()
        for _ in range(a.forward_iters):
            unet(x[:n], 500, encoder_hidden_states=ehs, pag_first=2 * B)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.forward_iters

    for r in range(a.rounds + 1):
        for k, (n, layers) in arms.items():
            ms = forward_ms(n, layers)
            if r:
                fw[k].append(ms)
    unet.set_pag_applied_layers("mid")
    med = {k: statistics.median(v) for k, v in fw.items()}
    res["forward"] = dict(h=h, w=w, iters=a.forward_iters, n16_ms=med["n16"], n24_mid_ms=med["n24_mid"], n24_all_ms=med["n24_all"],
                          runs=fw, ratio_mid=med["n24_mid"] / med["n16"], ratio_all=med["n24_all"] / med["n16"])
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
                                   7.5, 1.0, False, True, return_device=True, out_uint8=True, pag_table=[a.pag_scale] * STEPS if on else None)
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
    res["call"] = {"what": "%dx%d, %d DDIM steps, CFG 7.5, pag_applied_layers mid" % (H, W, STEPS), "iters": a.iters, "warmup": a.warmup}
    for on, name in ((False, "off"), (True, "on")):
        arm = call[on]
        sec = statistics.median(arm["seconds"])
        res["call"][name] = dict(loop_ms=statistics.median(arm["loop_ms"]), loop_ms_runs=arm["loop_ms"], seconds=sec, seconds_runs=arm["seconds"],
                                 images_per_s=B / sec)
    res["call"]["loop_ratio"] = res["call"]["on"]["loop_ms"] / res["call"]["off"]["loop_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
