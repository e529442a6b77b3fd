"""FreeU (`enable_freeu`) against the plain UNet, on one GPU: what the six extra launches of a whole forward cost.

    forward   the CFG forward of B = 8 (n = 16 samples of 64x48) timed with unet.time_forward, FreeU off / on / off / on ... interleaved in
              one process on one UNet (--rounds pairs after one untimed pair)
    call      512x384, B = 8, 50 DDIM steps, CFG 7.5 (BASELINE configs[1] shape): the fused run as bench.py runs it, one pipeline (one
              native handle, so its graphs stay captured) per arm, off / on interleaved: --warmup untimed rounds, then --iters timed ones

Full-size random-init checkpoint and bench.py's synthetic rows.  FreeU adds one launch per site, 2 * (layers_per_block + 1) = 6 per whole
forward (reported as launches_added: it is the definition, not a count taken from the device).  Image quality on real weights is NOT
evaluated here: the checkpoint is random-init.  Prints one JSON line.

    python tools/bench_freeu.py [--batch 8] [--rounds 3] [--forward-iters 10] [--iters 1] [--warmup 1] [--freeu 0.9 0.2 1.4 1.6]
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
    p.add_argument("--freeu", type=float, nargs=4, default=[0.9, 0.2, 1.4, 1.6], metavar=("S1", "S2", "B1", "B2"))
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
    freeu = tuple(a.freeu)

    def set_state(on):
        unet.enable_freeu(*freeu) if on else unet.disable_freeu()

    res = {"metric": "freeu_forward_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "freeu": freeu,
           "launches_added": 2 * (ucfg["layers_per_block"] + 1)}
    # ---- the forward alone
    n, h, w = 2 * B, H // 8, W // 8
    unet.set_context(torch.zeros((n, 77, D), dtype=torch.float16, device=dev))
    fw = {False: [], True: []}
    for r in range(a.rounds + 1):
        for on in (False, True):
            set_state(on)
            ms = unet.time_forward(n, h, w, a.forward_iters)
            if r:
                fw[on].append(ms)
    off, on_ = statistics.median(fw[False]), statistics.median(fw[True])
    res["forward"] = dict(n=n, h=h, w=w, iters=a.forward_iters, off_ms=off, on_ms=on_, off_ms_runs=fw[False], on_ms_runs=fw[True],
                          added_ms=on_ - off, added_pct=100.0 * (on_ - off) / off)
    # ---- the whole call
    rows = bench.make_rows(0, B, H, W, 77, D, dev)
    arms = {}
    for on in (False, True):
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
        arms[on] = dict(pipe=pipe, loop_ms=[], seconds=[])
    for r in range(a.warmup + a.iters):
        for on in (False, True):
            arm = arms[on]
            set_state(on)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arm["pipe"]._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                                   rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS,
                                   7.5, 1.0, False, True, return_device=True, out_uint8=True)
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
    set_state(False)
    res["call"] = {"what": "%dx%d, %d DDIM steps, CFG 7.5" % (H, W, STEPS), "iters": a.iters, "warmup": a.warmup}
    for on, name in ((False, "off"), (True, "on")):
        arm = arms[on]
        sec = statistics.median(arm["seconds"])
        res["call"][name] = dict(loop_ms=statistics.median(arm["loop_ms"]), loop_ms_runs=arm["loop_ms"], seconds=sec, seconds_runs=arm["seconds"],
                                 images_per_s=B / sec)
    res["call"]["loop_added_pct"] = 100.0 * (res["call"]["on"]["loop_ms"] - res["call"]["off"]["loop_ms"]) / res["call"]["off"]["loop_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
