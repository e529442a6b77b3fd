"""fp16 head-room report of a checkpoint: runs one try-on batch under a RangeProbe and prints, per named activation of UNet, VAE and EMASC,
the largest finite magnitude, its share of the fp16 range (65504) and the number of inf / NaN elements -- least head-room first.

    python tools/range_report.py                          # the synthetic (random-init) checkpoint of the released architecture
    python tools/range_report.py --checkpoint-dir DIR      # released state_dicts: DIR/unet.pth, DIR/vae.pth, DIR/emasc.pth (io.py)
    python tools/range_report.py --size tiny --steps 3     # a quick look: the tiny configuration at 128 x 128, 8 prompt tokens
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# --height / --width / --tokens when not given: what the configuration is meant for
SIZE_DEFAULTS = {"full": {"height": 512, "width": 384, "tokens": 77}, "tiny": {"height": 128, "width": 128, "tokens": 8}}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint-dir", default=None)
    ap.add_argument("--size", choices=sorted(SIZE_DEFAULTS), default="full")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--tokens", type=int, default=None, help="prompt length")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--execution-order", action="store_true", help="print the points in execution order instead of by head-room")
    a = ap.parse_args(argv)
    if a.checkpoint_dir and a.size != "full":
        ap.error("--checkpoint-dir holds the released architecture: --size tiny does not apply")
    for k, v in SIZE_DEFAULTS[a.size].items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    if a.height % 8 or a.width % 8 or a.height < 8 or a.width < 8:
        ap.error("--height and --width have to be positive multiples of 8")
    if a.batch < 1 or a.steps < 1 or a.tokens < 1:
        ap.error("--batch, --steps and --tokens have to be at least 1")
    return a


def render(report, first, execution_order=False):
    """the text the tool prints for a RangeProbe.report() and the name first_nonfinite() gave (or None)"""
    from ladi_vton_amd.probe import RangeProbe
    return "%s\n\nfirst non-finite activation: %s" % (RangeProbe.format(report, sort_by_headroom=not execution_order), first or "none")


def main(argv=None):
    a = parse_args(argv)
    import ladi_vton_amd as L
    from ladi_vton_amd import configs as C
    from ladi_vton_amd.io import load_released_state_dict
    from oracle.pipeline import synthetic_inputs
    if a.checkpoint_dir:
        ucfg, vcfg = C.UNET_FULL, C.VAE_FULL
        ecfg = C.emasc_for_vae(vcfg)
        sd = {k: load_released_state_dict(os.path.join(a.checkpoint_dir, k + ".pth")) for k in ("unet", "vae", "emasc")}
        pipe = L.StableDiffusionTryOnePipeline(vae=L.NativeVAE(vcfg, sd["vae"]), text_encoder=None, tokenizer=None, unet=L.NativeUNet(ucfg, sd["unet"]),
                                               scheduler=L.DDIMScheduler(), emasc=L.NativeEMASC(ecfg, sd["emasc"]), emasc_int_layers=[1, 2, 3, 4, 5])
    else:
        pipe, cfgs = L.build_random_init_pipeline(a.size, "ddim")
        ucfg = cfgs["unet"]
    probe = L.RangeProbe()
    pipe.range_probe = probe
    inp = synthetic_inputs(a.batch, a.height, a.width, L=a.tokens, D=ucfg["cross_attention_dim"])
    d = torch.device("cuda", 0)
    pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].to(d), pose_map=inp["pose_map"].to(d), warped_cloth=inp["warped_cloth"].to(d),
         prompt_embeds=inp["prompt_embeds"].half().to(d), negative_prompt_embeds=inp["negative_prompt_embeds"].half().to(d), height=a.height,
         width=a.width, num_inference_steps=a.steps, guidance_scale=a.guidance, output_type="np",
         noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]))
    first = probe.first_nonfinite()
    print(render(probe.report(), first, a.execution_order))
    return 1 if first else 0


if __name__ == "__main__":
    sys.exit(main())
