"""ms per batch of the fused try-on pipeline (ladi_tryon_run, hipGraph replay) at several image sizes: the full-size random-init checkpoint,
B = 8, 50 PNDM steps (51 UNet evaluations), guidance 7.5, EMASC on.  512x384 and 1024x768 have latents that are multiples of 8; 640x480
and 480x360 do not (the upsamplers stretch to the skips' sizes, diffusers' `forward_upsample_size`).

    python tools/bench_resolutions.py [--batch 8] [--runs 3] [--sizes 512x384,640x480] [--out FILE]

Every size runs once untimed (graph capture, per-shape tile measurement), then --runs times, each fenced by a device synchronise; the
median is reported, with ms per latent pixel per UNet evaluation (batch median / 51 / (B * h * w), h x w the latent) -- the whole loop's
cost spread over the evaluations, VAE and EMASC included."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ups_convs(n, iters):
    """the three upsampler convolutions of a 640x480 forward (n samples: 2 x batch with guidance) with the UNet's descriptors -- size-mapped
    nearest (10x8 -> 20x15, 20x15 -> 40x30, 40x30 -> 80x60) + 3x3 conv, bias, fused output statistics (the same tune key, so the same tile
    choice as in a forward) -- one untimed launch, then `iters` launches between HIP events.  The first launch of a shape the tile table
    does not hold is measured by the tuner (candidate launches); run once with LADI_TUNE_CACHE=<file> to record the choices, then again
    with the same file under rocprofv3 --kernel-trace --stats, so that the profiled process launches nothing but these convolutions."""
    import ctypes
    import torch
    from ladi_vton_amd import _lib
    from ladi_vton_amd._lib import IGemmDesc, stream_ptr
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    res = []
    for (hs, ws), (ho, wo), cin in (((10, 8), (20, 15), 1280), ((20, 15), (40, 30), 1280), ((40, 30), (80, 60), 640)):
        x = torch.randn((n, hs, ws, cin), device=dev).half()
        w = (torch.randn((cin, 9 * cin), device=dev) * 0.02).half()
        b = (torch.randn((cin,), device=dev) * 0.1).half()
        out = torch.empty((n, ho, wo, cin), device=dev, dtype=torch.float16)
        stats = torch.empty(((n * ho * wo + 31) // 32) * cin * 2, device=dev)     # worst case, as the runtime's alloc_part
        d = IGemmDesc()
        d.src0, d.C0, d.ld0 = x.data_ptr(), cin, cin
        d.Hs, d.Ws, d.Ho, d.Wo, d.P = hs, ws, ho, wo, n * ho * wo
        d.ksize, d.stride, d.pad, d.ups = 3, 1, 1, 1
        d.W, d.Q, d.K, d.ldw, d.out_scale = w.data_ptr(), cin, 9 * cin, 0, 1.0
        d.out, d.ldo, d.bias, d.stats = out.data_ptr(), cin, b.data_ptr(), stats.data_ptr()
        rc = lib.ladi_op_igemm(ctypes.byref(d), 1, 0, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            lib.ladi_op_igemm(ctypes.byref(d), 1, 0, stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        r = dict(src=[hs, ws], dst=[ho, wo], channels=cin, n=n, us_per_launch=round(1e3 * e0.elapsed_time(e1) / iters, 1))
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ups-convs", type=int, default=0, help="only time the 640x480 upsampler convolutions, this many launches each")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--sizes", default="512x384,640x480,480x360,1024x768")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import ladi_vton_amd as L
    from oracle import configs as C
    if a.ups_convs:
        torch.cuda.set_device(0)
        res = ups_convs(2 * a.batch, a.ups_convs)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(command="python tools/bench_resolutions.py " + " ".join(sys.argv[1:]), results=res), f, indent=1)
        return
    from oracle import pipeline as P
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ucfg, vcfg, ecfg = C.UNET_FULL, C.VAE_FULL, C.EMASC_FULL
    unet = L.NativeUNet(ucfg, C.synth_items(C.unet_shapes(ucfg), "unet."))
    vae = L.NativeVAE(vcfg, C.synth_items(C.vae_shapes(vcfg), "vae."))
    emasc = L.NativeEMASC(ecfg, C.synth_items(C.emasc_shapes(ecfg), "emasc."))
    B, steps = a.batch, a.steps
    results = []
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        inp = P.synthetic_inputs(B, H, W, L=77, D=1024)
        inp = {k: v.to(dev) for k, v in inp.items()}
        pe16 = inp["prompt_embeds"].half()
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.PNDMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])

        def run():
            return pipe._run_fused(inp["image"], inp["mask_image"], inp["pose_map"], inp["warped_cloth"], pe16, inp["negative_prompt_embeds"],
                                   inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"], H, W, steps, 7.5, 1.0, False, True,
                                   return_device=True, out_uint8=True)
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
        med = statistics.median(ms)
        evals = steps + 1
        h, w = H // 8, W // 8
        r = dict(height=H, width=W, latent=[h, w], latent_multiple_of_8=(h % 8 == 0 and w % 8 == 0), batch=B, scheduler="pndm", steps=steps,
                 unet_evaluations=evals, ms_per_batch_median=round(med, 1), ms_per_batch_runs=[round(v, 1) for v in ms],
                 images_per_s=round(B / (med / 1e3), 2), us_per_latent_pixel_per_evaluation=round(1e3 * med / evals / (B * h * w), 4))
        print(json.dumps(r), flush=True)
        results.append(r)
        del pipe
    out = dict(device=torch.cuda.get_device_name(0), command="python tools/bench_resolutions.py " + " ".join(sys.argv[1:]), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
