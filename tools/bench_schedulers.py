"""ms per batch of the fused try-on pipeline (ladi_tryon_run, hipGraph replay) for several schedulers on the same models and inputs:
the full-size random-init checkpoint, B = 8 at 512x384, guidance 7.5, EMASC on -- the shape of BASELINE configs[1], whose PNDM at 50
steps costs 51 UNet evaluations per image.

    python tools/bench_schedulers.py [--batch 8] [--runs 5] [--out FILE]

Every case runs once untimed (graph capture, per-shape tile measurement), then --runs times, each fenced by a device synchronise; the
median is reported.  Results stay on the device (uint8 images from the decode epilogue, as bench.py times them).  Euler-ancestral's
per-step noise is drawn before the timed region."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("pndm", 50), ("dpmpp_2m", 25), ("dpmpp_2m", 20), ("euler_ancestral", 25)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=384)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import ladi_vton_amd as L
    from oracle import configs as C
    from oracle import pipeline as P
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg, vcfg, ecfg = C.UNET_FULL, C.VAE_FULL, C.EMASC_FULL
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    B, H, W = a.batch, a.height, a.width
    inp = P.synthetic_inputs(B, H, W, L=77, D=1024)
    inp = {k: v.to(dev) for k, v in inp.items()}
    pe16 = inp["prompt_embeds"].half()
    make = {"pndm": L.PNDMScheduler, "dpmpp_2m": L.DPMSolverMultistepScheduler, "euler_ancestral": L.EulerAncestralDiscreteScheduler}
    results = []
    for name, steps in CASES:
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=make[name](), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
        noise = None
        if name == "euler_ancestral":
            g = torch.Generator(device=dev).manual_seed(0)
            noise = torch.randn((steps, B, 4, H // 8, W // 8), generator=g, device=dev)

        def run():
            return pipe._run_fused(inp["image"], inp["mask_image"], inp["pose_map"], inp["warped_cloth"], pe16, inp["negative_prompt_embeds"],
                                   inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, steps, 7.5, 1.0, False, True,
                                   return_device=True, out_uint8=True, step_noise=noise)
        run()
        torch.cuda.synchronize()
        if pipe.check_overflow():
            run()
            torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        evals = steps + 1 if name == "pndm" else steps
        med = statistics.median(ms)
        r = dict(scheduler=name, steps=steps, unet_evaluations=evals, batch=B, height=H, width=W, ms_per_batch_median=round(med, 1),
                 ms_per_batch_runs=[round(v, 1) for v in ms], images_per_s=round(B / (med / 1e3), 2))
        print(json.dumps(r), flush=True)
        results.append(r)
        del pipe
    out = dict(device=torch.cuda.get_device_name(0), command="python tools/bench_schedulers.py " + " ".join(sys.argv[1:]), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
