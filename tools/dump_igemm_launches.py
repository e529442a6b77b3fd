"""Record the implicit-GEMM launches of the product -> tests/golden/igemm_product_launches.txt (needs the GPU).

Switches the launch log on (ladi_igemm_launch_log, include/ladi_native.h) and runs the full-architecture modules on the deterministic
synthetic checkpoint (oracle.configs.synth_state_dict, as tests/test_gpu_e2e.py builds them):
    b8     BASELINE configs[1]: B = 8,  512x384, fused loop, graph on, 2 scheduler steps
    b32    BASELINE configs[2]: B = 32, 512x384, the same
    hr     BASELINE configs[4]: B = 1,  1024x768, the same
    text / vision / adapter / refine / tps   one call each of the other modules at their full configurations (fp16 callers)
and writes the distinct log lines, sorted, each behind the comma-separated tags of the runs it appeared in.  The repeat count is dropped:
a line is a launch FORM (geometry, operands present, key, configuration, source, what the launcher did), never a pointer or a value.
tests/tuned_cases.py parses the file; tests/test_gpu_tuned.py reruns `b8` and compares.  Reads nothing outside the repository.

    python tools/dump_igemm_launches.py [--only b8] [--out FILE]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_product_launches.txt")
TRYON_RUNS = dict(b8=(8, 512, 384), b32=(32, 512, 384), hr=(1, 1024, 768))
RUNS = ["b8", "b32", "hr", "text", "vision", "adapter", "refine", "tps"]
HEADER = """# distinct implicit-GEMM launches of the product, written by tools/dump_igemm_launches.py: <runs>\\t<launch form>
# src=1 lines of the runs b8 and b32 are rows of the shipped table: reproducible.  A src=2 line holds the configuration ONE capture measured for a
# shape the table lacks (1024x768, the encoders, the warping modules): timing decides it, so another capture may record another cfg there.  A
# src=1 line whose key the table lacks was served from such a measurement of an earlier run of the same capture.
"""


def read_log(lib):
    """the launch log as a list of lines without their repeat count"""
    n = lib.ladi_igemm_launch_log_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.ladi_igemm_launch_log_read(buf, n + 1)
    return [ln.rsplit(" n=", 1)[0] for ln in buf.value.decode().splitlines() if ln]


def tryon_modules():
    """the full-architecture UNet / VAE / EMASC on the synthetic checkpoint (tests/test_gpu_e2e.py `full`)"""
    import ladi_vton_amd as L
    from oracle import configs as C
    ucfg, vcfg, ecfg = C.UNET_FULL, C.VAE_FULL, C.EMASC_FULL
    return dict(unet=L.NativeUNet(ucfg, C.synth_state_dict(C.unet_shapes(ucfg), "unet.")),
                vae=L.NativeVAE(vcfg, C.synth_state_dict(C.vae_shapes(vcfg), "vae.")),
                emasc=L.NativeEMASC(ecfg, C.synth_state_dict(C.emasc_shapes(ecfg), "emasc.")))


def run_tryon(mod, B, H, W, steps=2):
    import ladi_vton_amd as L
    from oracle import pipeline as P
    inp = P.synthetic_inputs(B, H, W, L=77, D=1024)
    d = torch.device("cuda", 0)
    pipe = L.StableDiffusionTryOnePipeline(vae=mod["vae"], text_encoder=None, tokenizer=None, unet=mod["unet"], scheduler=L.PNDMScheduler(),
                                           emasc=mod["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])
    pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
         warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].half().to(d),
         negative_prompt_embeds=inp["negative_prompt_embeds"].half().to(d), height=H, width=W, num_inference_steps=steps,
         guidance_scale=7.5, output_type="np", fused=True, use_graph=True,
         noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    torch.cuda.synchronize()


def run_text():
    import ladi_vton_amd as L
    from oracle import configs as C
    cfg = C.TEXT_FULL
    enc = L.NativeCLIPTextEncoder(cfg, C.synth_state_dict(C.text_shapes(cfg), "text."))
    B, T, NV = 2, 77, 16
    g = torch.Generator().manual_seed(21)
    ids = torch.zeros((B, T), dtype=torch.int32)
    ids[:, 0] = 49406
    for b in range(B):
        ids[b, 1:9 + b] = torch.randint(300, 40000, (8 + b,), generator=g).int()
        ids[b, 9 + b:9 + b + NV] = 259
        ids[b, 9 + b + NV] = 49407
    we = torch.randn((B, NV, cfg["hidden"]), generator=g).half().float() * 0.05
    L.encode_text_word_embedding(enc, ids, we.to(torch.device("cuda", 0)), NV)
    torch.cuda.synchronize()


def run_vision():
    import ladi_vton_amd as L
    from oracle import configs as C
    cfg = C.VISION_FULL
    enc = L.NativeCLIPVisionEncoder(cfg, C.synth_state_dict(C.vision_shapes(cfg), "vision."))
    px = (torch.randn((2, 3, 224, 224), generator=torch.Generator().manual_seed(31)) * 1.2).half().float()
    enc(px.to(torch.device("cuda", 0)))
    torch.cuda.synchronize()


def run_adapter():
    import ladi_vton_amd as L
    from oracle import configs as C
    cfg = C.ADAPTER_FULL
    ad = L.NativeInversionAdapter(cfg, C.synth_state_dict(C.adapter_shapes(cfg), "adapter."))
    x = torch.randn((3, 257, 1280), generator=torch.Generator().manual_seed(11)).half()
    ad(x.to(torch.device("cuda", 0)))
    torch.cuda.synchronize()


def run_refine():
    import ladi_vton_amd as L
    from oracle import configs as C
    cfg = C.REFINE_FULL
    net = L.NativeRefinementUNet(cfg, C.synth_state_dict(C.refine_shapes(cfg), "refine.", fp16_round=False))
    x = torch.randn((2, 24, 512, 384), generator=torch.Generator().manual_seed(41)).half()
    net(x.to(torch.device("cuda", 0)))
    torch.cuda.synchronize()


def run_tps():
    import ladi_vton_amd as L
    from oracle import configs as C
    cfg = C.TPS_FULL
    tps = L.NativeTPS(cfg, C.synth_state_dict(C.tps_shapes(cfg), "tps.", fp16_round=False))
    g = torch.Generator().manual_seed(51)
    cloth = torch.randn((2, 3, 256, 192), generator=g).half()
    agnostic = torch.randn((2, cfg["input_nc"], 256, 192), generator=g).half()
    tps(cloth.to(torch.device("cuda", 0)), agnostic.to(torch.device("cuda", 0)))
    torch.cuda.synchronize()


def drop_served_after_measured(lines):
    """a shape the shipped table does not hold is measured by its first launch (src=2) and served from the process's table afterwards (src=1):
    the same launch form twice.  Only the first is a fact about the shipped table, so the second is dropped."""
    measured = {ln.replace(" src=2 ", " src=1 ") for ln in lines if " src=2 " in ln}
    return [ln for ln in lines if ln not in measured]


def capture(lib, fn):
    """the distinct launch forms of one run"""
    lib.ladi_igemm_launch_log(1)
    try:
        fn()
    finally:
        lib.ladi_igemm_launch_log(0)
    return drop_served_after_measured(read_log(lib))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(RUNS))
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from ladi_vton_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    torch.cuda.set_device(0)
    runs = args.only.split(",") if args.only else RUNS
    others = dict(text=run_text, vision=run_vision, adapter=run_adapter, refine=run_refine, tps=run_tps)
    tags = {}
    mod = tryon_modules() if any(r in TRYON_RUNS for r in runs) else None
    for r in runs:
        fn = (lambda r=r: run_tryon(mod, *TRYON_RUNS[r])) if r in TRYON_RUNS else others[r]
        lines = capture(lib, fn)
        for ln in lines:
            tags.setdefault(ln, []).append(r)
        print("%-8s %4d distinct launches" % (r, len(lines)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(HEADER)
        for ln in sorted(tags):
            fh.write("%s\t%s\n" % (",".join(tags[ln]), ln))
    print("%d distinct launch forms -> %s" % (len(tags), args.out))


if __name__ == "__main__":
    main()
