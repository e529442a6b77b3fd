"""Deep-feature cache (`feature_cache=`, DeepCache on the full-resolution level) against the plain run, on one GPU.

    plain     512x384, B = 8, 50 DDIM and 50 PNDM steps (BASELINE configs[1] shape): the fused run as bench.py runs it
    cached    the same run with a whole UNet evaluation every --interval-th and the others shallow at --branch (0, 1, 2)

Full-size random-init checkpoint and bench.py's synthetic rows.  Every arm has its own native handle (its graphs stay captured), the arms of a
scheduler are interleaved (plain, cached .., plain, cached ..) for --iters repetitions after --warmup untimed rounds, in one process.  Per arm:
the denoising-loop time (the library's stage events), the whole call's HIP-event time and images/s (median, every run listed), shallow_evals,
and -- information only -- the PSNR of the arm's final latents against the plain arm's.  Then the whole and the shallow UNet forward alone at
n = 16 samples of 64x48 (stand-alone launches, as bench.py's roofline leg times the forward).  Image quality on real weights is NOT evaluated
here: the checkpoint is random-init, so the drift figures say nothing about pictures.  Prints one JSON line.
Memory: the 1 + len(--interval) * len(--branch) handles of ONE scheduler are alive at a time (each with its B = 8 activation arena, its graphs
and a 31 / 63 MB cache; the default 10 handles fit an MI355X with room to spare); they are released before the next scheduler's are built.

    python tools/bench_feature_cache.py [--batch 8] [--iters 3] [--warmup 1] [--interval 2 3 5] [--branch 0 1 2] [--schedulers ddim pndm]
"""
import argparse
import ctypes
import gc
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, STEPS = 512, 384, 50
# SURVEY.md App. D census at 64x48, GFLOP per sample: the whole forward and a shallow evaluation at branch 0 / 1 / 2
FLOP_WHOLE, FLOP_SHALLOW = 581.7, {0: 43.8, 1: 123.3, 2: 209.1}


def psnr(a, b):
    a, b = a.double(), b.double()
    mse = float(((a - b) ** 2).mean())
    return None if mse == 0 else 10.0 * math.log10(float(b.abs().max()) ** 2 / mse)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--interval", type=int, nargs="+", default=[2, 3, 5])
    p.add_argument("--branch", type=int, nargs="+", default=[0, 1, 2])
    p.add_argument("--schedulers", nargs="+", default=["ddim", "pndm"], choices=["ddim", "pndm"])
    p.add_argument("--forward-iters", type=int, default=10)
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
    rows = bench.make_rows(0, B, H, W, 77, D, dev)

    res = {"metric": "feature_cache_seconds_per_batch", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0),
           "what": "%dx%d, %d steps, CFG 7.5" % (H, W, STEPS), "iters": a.iters, "warmup": a.warmup, "schedulers": {}}
    for sched in a.schedulers:
        def pipe():      # one native handle per arm: no arm re-captures its graphs when another has run
            return L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet,
                                                   scheduler=L.DDIMScheduler() if sched == "ddim" else L.PNDMScheduler(), emasc=emasc,
                                                   emasc_int_layers=[1, 2, 3, 4, 5])
        evals = STEPS + 1 if sched == "pndm" else STEPS
        arms = [dict(name="plain", interval=1, branch=0, pipe=pipe(), fc=None)]
        for n in a.interval:
            for k in a.branch:
                arms.append(dict(name="interval %d, branch %d" % (n, k), interval=n, branch=k, pipe=pipe(),
                                 fc=(L.feature_cache_plan(evals, n), k)))
        for arm in arms:
            arm.update(loop_ms=[], seconds=[])

        def run(arm, timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arm["pipe"]._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                                   rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS,
                                   7.5, 1.0, False, True, return_device=True, out_uint8=True, feature_cache=arm["fc"])
            e1.record()
            torch.cuda.synchronize()
            if arm["pipe"].check_overflow():
                raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
            if timed:
                ms = (ctypes.c_float * 3)()
                if lib.ladi_tryon_stage_ms(arm["pipe"]._tryon, ms) != 0:
                    raise RuntimeError("no stage times")
                arm["loop_ms"].append(ms[1])
                arm["seconds"].append(e0.elapsed_time(e1) / 1e3)
        for r in range(a.warmup + a.iters):      # interleaved: every round runs every arm once
            for arm in arms:
                run(arm, r >= a.warmup)
        plain = arms[0]
        lat0 = plain["pipe"].last_latents.float().cpu()
        out = []
        for arm in arms:
            loop, sec = statistics.median(arm["loop_ms"]), statistics.median(arm["seconds"])
            shallow = arm["pipe"].shallow_evals
            e = dict(arm=arm["name"], interval=arm["interval"], branch=arm["branch"], shallow_evals=shallow, evals=evals, loop_ms=loop,
                     loop_ms_runs=arm["loop_ms"], seconds=sec, seconds_runs=arm["seconds"], images_per_s=B / sec,
                     loop_time_ratio=loop / statistics.median(plain["loop_ms"]),
                     flop_ratio=((evals - shallow) * FLOP_WHOLE + shallow * FLOP_SHALLOW[arm["branch"]]) / (evals * FLOP_WHOLE),
                     latents_psnr_vs_plain_db=(None if arm is plain else psnr(arm["pipe"].last_latents.float().cpu(), lat0)))
            e["below_plain"] = bool(arm is plain or loop < statistics.median(plain["loop_ms"]))
            out.append(e)
        res["schedulers"][sched] = out
        del arms, plain, arm      # the handles (arenas, graphs, caches) of this scheduler go before the next scheduler's are built
        gc.collect()
        torch.cuda.synchronize()

    # the forwards alone, n = 16 (the CFG batch of B = 8) at 64x48
    n, h, w = 16, H // 8, W // 8
    unet.set_context(torch.zeros((n, 77, D), dtype=torch.float16, device=dev))
    whole = unet.time_forward(n, h, w, a.forward_iters)
    fw = {"n": n, "whole_ms": whole, "capture_ms": unet.time_forward_cached(n, h, w, a.forward_iters, "capture", 0), "shallow": []}
    for k in a.branch:
        ms = unet.time_forward_cached(n, h, w, a.forward_iters, "reuse", k)
        fw["shallow"].append(dict(branch=k, ms=ms, time_share=ms / whole, flop_share=FLOP_SHALLOW[k] / FLOP_WHOLE))
    res["forward"] = fw
    print(json.dumps(res))


if __name__ == "__main__":
    main()
