"""ms per batch of the try-on pipeline's public call with step callbacks and with DDIM's eta, on the full-size random-init checkpoint,
B = 8 at 512x384, guidance 7.5, EMASC on (the shape of tools/bench_schedulers.py):

  * PNDM 50 steps, fused: no callback, a no-op callback at callback_steps = 1 and at callback_steps = 10
  * DDIM 50 steps, fused: eta = 0 and eta = 1.0 (the per-step draws come from a seeded device generator inside the call)
  * PNDM 50 steps, module by module, with the same no-op callback (for comparison)
  * PNDM 50 steps, fused, no callback, once more at the end: how far the box drifted over the run

    python tools/bench_callbacks.py [--batch 8] [--runs 5] [--modular-runs 2] [--out FILE]

Every case runs once untimed (graph capture, per-shape tile measurement), then its runs, each fenced by a device synchronise; the median
is reported.  Every case goes through StableDiffusionTryOnePipeline.__call__ with output_type="np", so the images reach the host in all of
them (unlike tools/bench_schedulers.py, which leaves uint8 images on the device)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, scheduler, steps, fused, eta, callback_steps (None: no callback)
CASES = [("pndm_no_callback", "pndm", 50, True, 0.0, None), ("pndm_callback_every_1", "pndm", 50, True, 0.0, 1),
         ("pndm_callback_every_10", "pndm", 50, True, 0.0, 10), ("ddim_eta_0", "ddim", 50, True, 0.0, None),
         ("ddim_eta_1", "ddim", 50, True, 1.0, None), ("pndm_modular_callback_every_1", "pndm", 50, False, 0.0, 1),
         ("pndm_no_callback_again", "pndm", 50, True, 0.0, None)]      # the first case once more: the drift over the whole run


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=384)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--modular-runs", type=int, default=2)
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
    make = {"pndm": L.PNDMScheduler, "ddim": L.DDIMScheduler}
    calls = []

    def noop(i, t, latents):
        calls.append(i)

    results = []
    for name, sched, steps, fused, eta, every in CASES:
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=make[sched](), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])

        def run():
            del calls[:]
            pipe(image=inp["image"], mask_image=inp["mask_image"].clone(), pose_map=inp["pose_map"], warped_cloth=inp["warped_cloth"],
                 prompt_embeds=inp["prompt_embeds"].half(), negative_prompt_embeds=inp["negative_prompt_embeds"].half(), height=H, width=W,
                 num_inference_steps=steps, guidance_scale=7.5, output_type="np", fused=fused, eta=eta,
                 generator=torch.Generator(device=dev).manual_seed(0), callback=noop if every else None, callback_steps=every or 1,
                 noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
        run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs if fused else a.modular_runs):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        evals = steps + 1 if sched == "pndm" else steps
        med = statistics.median(ms)
        r = dict(case=name, scheduler=sched, steps=steps, unet_evaluations=evals, path="fused" if fused else "modular", eta=eta,
                 callback_steps=every, callback_calls_per_batch=len(calls), batch=B, height=H, width=W, ms_per_batch_median=round(med, 1),
                 ms_per_batch_runs=[round(v, 1) for v in ms], images_per_s=round(B / (med / 1e3), 2))
        print(json.dumps(r), flush=True)
        results.append(r)
        del pipe
    out = dict(device=torch.cuda.get_device_name(0), command="python tools/bench_callbacks.py " + " ".join(sys.argv[1:]), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
