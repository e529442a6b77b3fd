"""Token merging (`apply_token_merging`) against the same binary with merging off, on one GPU.

    kernels   every new kernel alone at the level-0 shape of each size (n = 2B samples, T = h w tokens, C = 320), HIP events around
              --kernel-iters launches: prep + match (ladi_op_tome_match; TFLOP/s over 2 Ns Nd C, prep included, so a lower bound for the
              match kernel), plan, merge, unmerge-add, next to flash_attn64 over the same T and over T - r
    forward   the CFG forward of B = 8 (n = 16) through NativeUNet.__call__, arms interleaved in one process on one UNet: off, then
              ratio 0.25 / 0.5 / 0.75 with merge_attn alone and with all three flags (--rounds after one untimed round)
    call      B = 8, 50 DDIM steps, CFG 7.5: the fused run as bench.py runs it, the same arms interleaved; every arm change re-captures the
              graphs (the configuration is part of the graph key), so each timed call follows an untimed one at the same configuration

Full-size random-init checkpoint and bench.py's synthetic rows.  Image quality on real weights is NOT evaluated here.  Prints one JSON line.

    python tools/bench_tome.py [--batch 8] [--sizes 512x384,1024x768] [--rounds 2] [--forward-iters 5] [--call-iters 1] [--no-call]
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

STEPS = 50
RATIOS = (0.25, 0.5, 0.75)


def arms():
    out = [("off", None)]
    for r in RATIOS:
        out.append(("attn_%g" % r, dict(ratio=r)))
        out.append(("all_%g" % r, dict(ratio=r, merge_crossattn=True, merge_mlp=True)))
    return out


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(lib, n, h, w, C, ratio, iters, dev):
    from ladi_vton_amd._lib import ptr, stream_ptr
    T = h * w
    sp, dp = (ctypes.c_int * T)(), (ctypes.c_int * T)()
    Nd = lib.ladi_tome_tables(h, w, 2, 2, 0, 0, sp, dp, T)
    Ns = T - Nd
    r = lib.ladi_tome_merge_count(T, Ns, ratio)
    Tm = T - r
    g = torch.Generator().manual_seed(1)
    x = torch.randn((n, T, C), generator=g).to(dev, torch.float16)
    dsp = torch.tensor(list(sp[:Ns]), dtype=torch.int32, device=dev)
    ddp = torch.tensor(list(dp[:Nd]), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ladi_op_tome_match_workspace_bytes(n, Ns, Nd, C) // 2, dtype=torch.float16, device=dev)
    score = torch.empty((n, Ns), dtype=torch.float32, device=dev)
    node = torch.empty((n, Ns), dtype=torch.int32, device=dev)
    orow = torch.empty((n, T), dtype=torch.int32, device=dev)
    plan = torch.empty((n, lib.ladi_op_tome_plan_ints(Ns, Nd, r)), dtype=torch.int32, device=dev)
    y = torch.empty((n, Tm, C), dtype=torch.float16, device=dev)
    out = torch.empty((n, T, C), dtype=torch.float16, device=dev)

    def ok(rc):
        if rc:
            raise RuntimeError("launch refused: rc %d" % rc)
    res = dict(n=n, T=T, Ns=Ns, Nd=Nd, r=r, C=C)
    ms = timed(lambda: ok(lib.ladi_op_tome_match(ptr(x), C, T * C, ptr(dsp), ptr(ddp), n, T, Ns, Nd, C, ptr(ws), ptr(score), ptr(node), stream_ptr())), iters)
    res["match_us"] = ms * 1e3
    res["match_tflops"] = 2.0 * n * Ns * Nd * C / (ms * 1e-3) / 1e12
    res["plan_us"] = 1e3 * timed(lambda: ok(lib.ladi_op_tome_plan(ptr(score), ptr(node), ptr(dsp), ptr(ddp), n, T, Ns, Nd, r, ptr(orow), ptr(plan), stream_ptr())), iters)
    res["merge_us"] = 1e3 * timed(lambda: ok(lib.ladi_op_tome_merge(ptr(x), C, T * C, ptr(ddp), ptr(plan), n, T, Ns, Nd, r, C, ptr(y), C, Tm * C, stream_ptr())), iters)
    res["unmerge_add_us"] = 1e3 * timed(lambda: ok(lib.ladi_op_tome_unmerge_add(ptr(y), C, Tm * C, ptr(x), C, T * C, ptr(orow), n, T, Tm, C, ptr(out), C, T * C,
                                                                                 stream_ptr())), iters)
    heads = C // 64
    qkv = torch.randn((n, T, 3 * C), generator=g).to(dev, torch.float16)
    o = torch.empty((n, T, C), dtype=torch.float16, device=dev)
    for name, Tq in (("flash_attn64_T_us", T), ("flash_attn64_Tm_us", Tm)):
        res[name] = 1e3 * timed(lambda: ok(lib.ladi_op_attention(ptr(qkv), ctypes.c_void_p(qkv.data_ptr() + 2 * C), ctypes.c_void_p(qkv.data_ptr() + 4 * C), ptr(o),
                                                                  3 * C, 3 * C, 3 * C, C, Tq * 3 * C, Tq * 3 * C, Tq * 3 * C, Tq * C, n, heads, Tq, Tq, 0.125,
                                                                  stream_ptr())), iters)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--sizes", default="512x384,1024x768")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--forward-iters", type=int, default=5)
    p.add_argument("--kernel-iters", type=int, default=20)
    p.add_argument("--call-iters", type=int, default=1)
    p.add_argument("--no-call", action="store_true")
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
    res = {"metric": "tome_ms", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0), "sizes": {}}

    def configure(cfg):
        unet.set_token_merging(**cfg) if cfg else unet.remove_token_merging()

    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        h, w = H // 8, W // 8
        out = res["sizes"][size] = {"kernels": {"%g" % r: kernels(lib, 2 * B, h, w, ucfg["block_out_channels"][0], r, a.kernel_iters, dev) for r in RATIOS}}
        g = torch.Generator().manual_seed(0)
        ehs = torch.randn((2 * B, 77, D), generator=g).to(dev, torch.float16)
        x = (torch.randn((2 * B, ucfg["in_channels"], h, w), generator=g) * 0.5).to(dev, torch.float16)
        fw = {k: [] for k, _ in arms()}
        for rnd in range(a.rounds + 1):
            for k, cfg in arms():
                configure(cfg)
                ms = timed(lambda: unet(x, 500, encoder_hidden_states=ehs), a.forward_iters)
                if rnd:
                    fw[k].append(ms)
        med = {k: statistics.median(v) for k, v in fw.items()}
        out["forward"] = {k: dict(ms=med[k], runs=fw[k], ratio_to_off=med[k] / med["off"]) for k in med}
        if a.no_call:
            continue
        rows = bench.make_rows(0, B, H, W, 77, D, dev)
        pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.DDIMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
        call = {k: [] for k, _ in arms()}

        def run():
            pipe._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                            rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS, 7.5, 1.0,
                            False, True, return_device=True, out_uint8=True)
            torch.cuda.synchronize()
            if pipe.check_overflow():
                raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
            ms = (ctypes.c_float * 3)()
            if lib.ladi_tryon_stage_ms(pipe._tryon, ms) != 0:
                raise RuntimeError("no stage times")
            return ms[1]
        for rnd in range(a.call_iters):
            for k, cfg in arms():
                configure(cfg)
                run()                               # captures this configuration's graphs
                call[k].append(run())
        med = {k: statistics.median(v) for k, v in call.items()}
        out["call_loop_ms"] = {k: dict(ms=med[k], runs=call[k], ratio_to_off=med[k] / med["off"]) for k in med}
    unet.remove_token_merging()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
