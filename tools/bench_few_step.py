"""Few-step sampling on one GPU: what a whole try-on call costs at 1 - 8 evaluations, next to the plain 50-step run of the same process.

Full-size random-init models, B = 8 at 512x384 (the flagship shape), the public pipeline call on the fused hipGraph path.  One case per row:

    ddim_50            the plain run: DDIM, 50 steps, guidance 7.5 -- the point of comparison, measured in this process
    lcm_N_g1 / _g7.5   LCMScheduler at N = 8, 4, 2, 1 steps, guidance 1.0 (cond-only: the UNet runs over the 8 conditional samples) and 7.5
    tcd_4_eta0.3       TCDScheduler, 4 steps, eta (gamma) 0.3, guidance 1.0
    euler_t_N          EulerDiscreteScheduler(timestep_spacing="trailing") at 1 and 4 steps, guidance 1.0

For each: the wall time of the call (host, synchronised, images on the host as numpy; median of --rounds after one untimed call) and the
device split of ladi_tryon_stage_ms: VAE encodes + EMASC, the denoising loop, the decode.  The models are random-init: the figures are costs,
the image quality of real distilled weights is not evaluated.

Prints one JSON line; --append FILE also appends the table in Markdown (with the commit and the device it was measured on).

    python tools/bench_few_step.py [--rounds 3] [--batch 8] [--size full] [--append BASELINE.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def commit():
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True, timeout=10)
        if out.returncode == 0 and out.stdout.strip():
            return out.stdout.strip() + ("+changes" if dirty.stdout.strip() else "")
    except (OSError, subprocess.SubprocessError):
        pass
    return "unknown (no git metadata)"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    p.add_argument("--commit", default=None, help="the commit the figures belong to (default: git rev-parse)")
    p.add_argument("--append", default=None, help="append the Markdown table to this file")
    a = p.parse_args()

    import ladi_vton_amd as L
    from oracle import pipeline as P
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    pipe, cfgs = L.build_random_init_pipeline(a.size)
    B, H, W = a.batch, 512, 384
    inp = P.synthetic_inputs(B, H, W, L=77, D=cfgs["unet"]["cross_attention_dim"])
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}

    cases = [("ddim_50", L.DDIMScheduler(), 50, 7.5, 0.0)]
    for n in (8, 4, 2, 1):
        for g in (1.0, 7.5):
            cases.append(("lcm_%d_g%g" % (n, g), L.LCMScheduler(), n, g, 0.0))
    cases.append(("tcd_4_eta0.3", L.TCDScheduler(), 4, 1.0, 0.3))
    for n in (1, 4):
        cases.append(("euler_t_%d" % n, L.EulerDiscreteScheduler(timestep_spacing="trailing"), n, 1.0, 0.0))

    def call(sch, n, g, eta):
        pipe.scheduler = sch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(image=inp["image"], mask_image=inp["mask_image"].clone(), pose_map=inp["pose_map"], warped_cloth=inp["warped_cloth"],
             prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], height=H, width=W,
             num_inference_steps=n, guidance_scale=g, eta=eta, output_type="np", generator=torch.Generator().manual_seed(1),
             noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, list(pipe.last_stage_ms)

    res = {"metric": "few_step_call_ms", "size": a.size, "device": torch.cuda.get_device_name(0), "commit": a.commit or commit(), "batch": B,
           "height": H, "width": W, "rounds": a.rounds, "cases": {}}
    for name, sch, n, g, eta in cases:
        call(sch, n, g, eta)                                       # untimed: tile measurement, arena, graph capture
        runs = [call(sch, n, g, eta) for _ in range(a.rounds)]
        med = lambda xs: statistics.median(xs)          # noqa: E731
        res["cases"][name] = dict(steps=n, guidance=g, eta=eta, unet_samples=(2 if g > 1.0 else 1) * B, cond_only_evals=pipe.cond_only_evals(),
                                  call_ms=med([r[0] for r in runs]), call_ms_runs=[r[0] for r in runs],
                                  encode_ms=med([r[1][0] for r in runs]), loop_ms=med([r[1][1] for r in runs]),
                                  decode_ms=med([r[1][2] for r in runs]))
    base = res["cases"]["ddim_50"]["call_ms"]
    for c in res["cases"].values():
        c["speedup_vs_ddim_50"] = base / c["call_ms"]
    print(json.dumps(res))
    if a.append:
        lines = ["", "### Few-step sampling (tools/bench_few_step.py)", "",
                 "Commit %s, %s, one process; B = %d at %dx%d, full-size random-init models, fused hipGraph path, median of %d calls after one"
                 % (res["commit"], res["device"], B, H, W, a.rounds),
                 "untimed call.  `call` is the host wall time of the pipeline call (images on the host); encode / loop / decode are the device",
                 "spans of `ladi_tryon_stage_ms`.  `ddim_50` is the plain run, measured in the same process.  Image quality on real distilled",
                 "weights: unevaluated.", "",
                 "| case | steps | guidance | UNet samples | call ms | encode ms | loop ms | decode ms | call vs ddim_50 |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for name, c in res["cases"].items():
            lines.append("| %s | %d | %g | %d | %.1f | %.1f | %.1f | %.1f | %.2fx |" % (
                name, c["steps"], c["guidance"], c["unet_samples"], c["call_ms"], c["encode_ms"], c["loop_ms"], c["decode_ms"],
                c["speedup_vs_ddim_50"]))
        with open(a.append, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
