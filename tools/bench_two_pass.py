"""Two-pass try-on against the plain configs[4] batch, on one GPU.

    plain     1024x768, 100 DDIM steps, B = 8 (BASELINE configs[4], single-GPU shard): one fused run
    two-pass  50 DDIM steps at 512x384, then the tail of the 100-step schedule at 1024x768 started from the low-resolution run's latents
              (init_latents = last_latents, resampled 64x48 -> 128x96 by the start-latents kernel) for each --strength

Full-size random-init checkpoint and bench.py's synthetic rows (the low-resolution pass sees the same rows, resized).  Times are HIP-event
times around the fused calls (results stay on the device, uint8 from the decode epilogue, as bench.py runs them) after --warmup untimed runs;
the median of --iters runs is reported, every run listed.  Prints one JSON line.  Image quality of the two-pass result is NOT evaluated here:
the checkpoint is random-init.

    python tools/bench_two_pass.py [--batch 8] [--iters 3] [--warmup 1] [--strength 0.3 0.5]
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

HI, LO = (1024, 768, 100), (512, 384, 50)      # (H, W, DDIM steps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--strength", type=float, nargs="+", default=[0.3, 0.5])
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    a = p.parse_args()

    import bench
    import ladi_vton_amd as L
    from oracle import configs as C
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg, vcfg = (C.UNET_FULL, C.VAE_FULL) if a.size == "full" else (C.UNET_TINY, C.VAE_TINY)
    ecfg = C.emasc_for_vae(vcfg)
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))

    def pipe():      # one native handle per resolution: neither re-plans its arena or re-captures its graph when the other runs
        return L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
    pipe_hi, pipe_lo = pipe(), pipe()
    B, D = a.batch, ucfg["cross_attention_dim"]
    hi = bench.make_rows(0, B, HI[0], HI[1], 77, D, dev)
    lo = bench.make_rows(0, B, LO[0], LO[1], 77, D, dev)
    F = torch.nn.functional
    for k in ("image", "pose_map", "warped_cloth"):
        lo[k] = F.interpolate(hi[k].float(), size=LO[:2], mode="bilinear", align_corners=False).half()
    lo["mask_image"] = F.interpolate(hi["mask_image"].float(), size=LO[:2]).half()
    lo["prompt_embeds"], lo["negative_prompt_embeds"] = hi["prompt_embeds"], hi["negative_prompt_embeds"]

    def run(pp, rows, size, **kw):
        return pp._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                             rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], size[0], size[1],
                             size[2], 7.5, 1.0, False, True, return_device=True, out_uint8=True, **kw)

    def plain():
        run(pipe_hi, hi, HI)

    def two_pass(strength):
        first = L.strength_first_step(strength, HI[2])
        run(pipe_lo, lo, LO)
        run(pipe_hi, hi, HI, init_latents=pipe_lo.last_latents, first_step=first)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / 1e3)
        if pipe_hi.check_overflow() or pipe_lo.check_overflow():
            raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
        return out

    res = {"metric": "two_pass_seconds_per_batch", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0),
           "plain": {"what": "%dx%d, %d DDIM steps" % HI}, "two_pass": []}
    t = timed(plain)
    res["plain"].update(seconds=statistics.median(t), runs=t, images_per_s=B / statistics.median(t))
    for s in a.strength:
        t = timed(lambda: two_pass(s))
        first = L.strength_first_step(s, HI[2])
        res["two_pass"].append({"strength": s, "what": "%dx%d, %d DDIM steps, then steps %d..%d of %d at %dx%d"
                                % (LO + (first, HI[2] - 1, HI[2]) + HI[:2]), "high_resolution_evaluations": HI[2] - first,
                                "seconds": statistics.median(t), "runs": t, "images_per_s": B / statistics.median(t),
                                "speedup_vs_plain": res["plain"]["seconds"] / statistics.median(t)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
