"""The tiny try-on pipeline the end-to-end GPU tests run: synthetic weights for UNET_TINY / VAE_TINY and their EMASC, the native modules, the
synthetic inputs and one pipeline call.  A plain module, no fixtures: every test file keeps its own module-scoped `tiny` fixture around
build(), so native modules are built once per test module and state set on a handle (FreeU, LoRA, token merging, an image-prompt adapter)
never reaches another file; its own `ref` and `run` caches live in the dict build() returns."""
import torch

from oracle import configs as C
from oracle import pipeline as P
from tests import strength_ref as SR
from tests import util as U

ARMS = {"graph": (True, True), "eager": (True, False), "modular": (False, False)}       # arm -> (fused, use_graph)


def build():
    import ladi_vton_amd as L
    ucfg, vcfg = C.UNET_TINY, C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    sds = dict(unet=C.synth_state_dict(C.unet_shapes(ucfg), "unet."), vae=C.synth_state_dict(C.vae_shapes(vcfg), "vae."),
               emasc=C.synth_state_dict(C.emasc_shapes(ecfg), "emasc."))
    mods = dict(unet=L.NativeUNet(ucfg, sds["unet"]), vae=L.NativeVAE(vcfg, sds["vae"]), emasc=L.NativeEMASC(ecfg, sds["emasc"]))
    return dict(ucfg=ucfg, vcfg=vcfg, ecfg=ecfg, sd=sds, mod=mods, ref={}, run={}, fwd={}, inp={})


def inputs(tiny, B, H, W):
    """oracle.pipeline.synthetic_inputs with 8 context tokens and fp16-representable embeddings, once per size"""
    if (B, H, W) not in tiny["inp"]:
        inp = P.synthetic_inputs(B, H, W, L=8, D=tiny["ucfg"]["cross_attention_dim"])
        for k in ("prompt_embeds", "negative_prompt_embeds"):
            inp[k] = inp[k].half().float()
        tiny["inp"][(B, H, W)] = inp
    return tiny["inp"][(B, H, W)]


def unet_inputs(tiny, hw, n=4):
    """-> (x, ehs, x on the device, ehs on the device).  n = 4: samples 2, 3 are copies of samples 0, 1, inputs and context alike; else n
    different samples"""
    key = (hw, n)
    if key not in tiny["fwd"]:
        g = torch.Generator().manual_seed(11 + hw[0])
        m = 2 if n == 4 else n
        x = torch.randn((m, 31) + hw, generator=g).half().float()
        ehs = torch.randn((m, 8, tiny["ucfg"]["cross_attention_dim"]), generator=g).half().float()
        if n == 4:
            x, ehs = torch.cat([x, x]), torch.cat([ehs, ehs])
        tiny["fwd"][key] = (x, ehs, x.to(U.dev()), ehs.to(U.dev()))
    return tiny["fwd"][key]


def pipe(tiny, scheduler="ddim"):
    """a fresh pipeline (a fresh native handle) over the shared native modules; scheduler: a name of strength_ref.SCHEDULERS"""
    import ladi_vton_amd as L
    return L.StableDiffusionTryOnePipeline(vae=tiny["mod"]["vae"], text_encoder=None, tokenizer=None, unet=tiny["mod"]["unet"],
                                           scheduler=SR.make_mirror(scheduler), emasc=tiny["mod"]["emasc"], emasc_int_layers=[1, 2, 3, 4, 5])


def call(tiny, pipe, inp, fused, graph, **kw):
    """one run at the inputs' size with their three noise draws -> (images [B, H, W, 3], final latents), fp32 on the host"""
    d = U.dev()
    H, W = inp["image"].shape[-2:]
    out = pipe(image=inp["image"].to(d), mask_image=inp["mask_image"].clone().to(d), pose_map=inp["pose_map"].to(d),
               warped_cloth=inp["warped_cloth"].to(d), prompt_embeds=inp["prompt_embeds"].to(d),
               negative_prompt_embeds=inp["negative_prompt_embeds"].to(d), height=H, width=W, output_type="np", fused=fused, use_graph=graph,
               noise=(inp["noise_cloth"], inp["noise_latents"], inp["noise_masked"]), **kw)
    return torch.from_numpy(out.images), pipe.last_latents.float().cpu()


def assert_close(what, img, lat, ref_img, ref_lat):
    """thresholds of test_tryon_pipeline_tiny: latents >= 40 dB, image >= 35 dB on [0, 1] -> (image dB, latents dB)"""
    p_img, p_lat = U.psnr(img, ref_img, peak=1.0), U.psnr(lat, ref_lat)
    print("%s: image %.2f dB, latents %.2f dB" % (what, p_img, p_lat))
    assert img.shape == ref_img.shape and torch.isfinite(lat).all()
    assert p_lat >= 40.0 and p_img >= 35.0, (what, p_img, p_lat)
    return p_img, p_lat
