"""images/s and stage times of the fused try-on pipeline (ladi_tryon_run, hipGraph replay) under the three guidance controls, on the shape of
BASELINE configs[1]: the full-size random-init checkpoint, B = 8 at 512x384, PNDM at 50 steps (51 UNet evaluations), EMASC on.

    python tools/bench_guidance.py [--arms a,b,c] [--runs 5] [--out FILE] [--root DIR]

  a  the scalar run, guidance_scale = 7.5 (what bench.py times)
  b  guidance_interval: CFG on the first 60 % of the evaluations, cond-only (B samples instead of 2B) on the rest
  c  guidance_rescale = 0.7 over all evaluations at the scalar scale

Every arm runs once untimed (graph capture, per-shape tile measurement), then the arms are INTERLEAVED: --runs rounds of one timed run per arm,
each fenced by a device synchronise; medians are reported, with ladi_tryon_stage_ms of the median run.  Results stay on the device (uint8
images from the decode epilogue, as bench.py times them).  Prints one JSON line.

--root DIR imports the package from another checkout (arm a only needs what every revision has): run this tool alternately with and
without it to compare the scalar run of two libraries on the same box in the same session."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=384)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--arms", default="a,b,c")
    p.add_argument("--root", default=ROOT)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    import ladi_vton_amd as L
    from ladi_vton_amd import _lib
    from oracle import configs as C
    from oracle import pipeline as P
    assert os.path.abspath(L.__file__).startswith(root + os.sep), L.__file__
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ucfg, vcfg, ecfg = C.UNET_FULL, C.VAE_FULL, C.EMASC_FULL
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    B, H, W, steps = a.batch, a.height, a.width, a.steps
    inp = {k: v.to(dev) for k, v in P.synthetic_inputs(B, H, W, L=77, D=1024).items()}
    pe16 = inp["prompt_embeds"].half()
    evals = steps + 1
    arms = [x for x in a.arms.split(",") if x]
    kwargs = {"a": {}}
    if "b" in arms:
        kwargs["b"] = dict(guidance_table=L.guidance_interval(evals, 7.5, 0.0, 0.6))
    if "c" in arms:
        kwargs["c"] = dict(guidance_rescale=0.7)
    # one pipeline (one native handle, its own captured graphs) per arm, on the same modules
    pipes = {x: L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.PNDMScheduler(), emasc=emasc,
                                                emasc_int_layers=[1, 2, 3, 4, 5]) for x in arms}

    def run(x):
        return pipes[x]._run_fused(inp["image"], inp["mask_image"], inp["pose_map"], inp["warped_cloth"], pe16, inp["negative_prompt_embeds"],
                                   inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, steps, 7.5, 1.0, False, True,
                                   return_device=True, out_uint8=True, **kwargs[x])

    def stage_ms(x):
        ms = (ctypes.c_float * 3)()
        return [round(v, 2) for v in ms] if lib.ladi_tryon_stage_ms(pipes[x]._tryon, ms) == 0 else None
    for x in arms:
        run(x)
        torch.cuda.synchronize()
        if pipes[x].check_overflow():
            run(x)
            torch.cuda.synchronize()
    rec = {x: [] for x in arms}
    for _ in range(a.runs):
        for x in arms:
            t0 = time.perf_counter()
            run(x)
            torch.cuda.synchronize()
            rec[x].append(((time.perf_counter() - t0) * 1e3, stage_ms(x)))
    res = {}
    for x in arms:
        ms = [r[0] for r in rec[x]]
        med = statistics.median(ms)
        res[x] = dict(ms_per_batch_median=round(med, 1), ms_per_batch_runs=[round(v, 1) for v in ms], images_per_s=round(B / (med / 1e3), 3),
                      stage_ms_preprocess_loop_decode=min(rec[x], key=lambda r: abs(r[0] - med))[1])
        if hasattr(pipes[x], "cond_only_evals"):
            res[x]["cond_only_evals"] = pipes[x].cond_only_evals()
    out = dict(tool="bench_guidance", device=torch.cuda.get_device_name(0), library_root=os.path.relpath(root, ROOT), batch=B, height=H, width=W,
               scheduler="pndm", steps=steps, unet_evaluations=evals, runs=a.runs, arms=res)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
