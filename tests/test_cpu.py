"""CPU-only tests: the oracle against the golden vectors / known-answer anchors, host logic of the product (schedulers,
input validation, sharding) and the C-ABI surface (library loads, exports every declared symbol; no compute without a GPU)."""
import ctypes
import json
import os
from collections import OrderedDict
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from ladi_vton_amd import configs as LC
from oracle import configs as C
from oracle import models as M
from oracle import pipeline as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------------------------------------------- oracle pins
def test_parameter_counts_match_known_sizes():
    """the restated module trees must reproduce the well-known sizes to the unit"""
    assert C.param_count(C.unet_shapes(C.UNET_FULL)) == 865_988_484
    assert C.param_count(C.unet_shapes(dict(C.UNET_FULL, in_channels=4))) == 865_910_724
    assert C.param_count(C.unet_shapes(dict(C.UNET_FULL, in_channels=9))) == 865_925_124
    assert C.param_count(C.vae_shapes(C.VAE_FULL)) == 83_653_863
    assert C.param_count(C.emasc_shapes(C.EMASC_FULL)) == 7_965_696
    assert C.param_count(C.adapter_shapes(C.ADAPTER_FULL)) == 136_360_704
    assert C.emasc_for_vae(C.VAE_FULL) == C.EMASC_FULL


def test_scheduler_known_answers():
    """SURVEY.md App. A.5 anchors"""
    ac = P.alphas_cumprod()
    for t, v in {0: 0.99914998, 1: 0.99829602, 21: 0.98038065, 961: 0.00728172, 981: 0.00577550, 999: 0.00466010}.items():
        assert abs(float(ac[t]) - v) < 2e-7 * max(1.0, v / 1e-3)
    d = P.DDIM(); d.set_timesteps(50)
    assert d.timesteps[:3] == [981, 961, 941] and d.timesteps[-2:] == [21, 1] and len(d.timesteps) == 50
    d.set_timesteps(20); assert d.timesteps[:3] == [951, 901, 851]
    d.set_timesteps(100); assert d.timesteps[:3] == [991, 981, 971]
    p = P.PNDM(); p.set_timesteps(50)
    assert p.timesteps[:4] == [981, 961, 961, 941] and p.timesteps[-1] == 1 and len(p.timesteps) == 51
    # product of the DDIM x-coefficients over 50 steps (how much the sampler alone amplifies a latent perturbation)
    d.set_timesteps(50)
    prod = 1.0
    for t in d.timesteps:
        tp = t - 20
        prod *= (float(ac[tp] if tp >= 0 else ac[0]) / float(ac[t])) ** 0.5
    assert abs(prod - 13.15) < 0.02


def test_oracle_matches_reference_emasc_fixture():
    """fixtures were produced by the REAL reference modules (oracle/make_golden.py): src/models/emasc.py, src/utils/data_utils.py"""
    g = load_file(os.path.join(GOLD, "emasc_tiny.safetensors"))
    sd = C.synth_state_dict(C.emasc_shapes(C.EMASC_TINY), "emasc.")
    outs = M.emasc_forward(sd, [g["feat%d" % i] for i in range(5)])
    for i in range(5):
        assert torch.allclose(outs[i], g["emasc%d" % i], atol=1e-5, rtol=1e-5)
    mk = M.mask_features(outs, g["mask"])
    for i in range(5):
        assert torch.allclose(mk[i], g["masked%d" % i], atol=1e-5, rtol=1e-5)


def test_oracle_matches_real_reference_vae_wiring():
    """tests/golden/ref_wiring.safetensors was produced by the REAL src/models/AutoencoderKL.py + src/models/vae.py Encoder / Decoder
    (oracle/make_golden.py:make_wiring_golden, diffusers blocks stood in by oracle/ref_harness.py): the oracle must reproduce the 6-entry
    feature list, the posterior, and the decoder's reverse() / `+=` order / int_layers index arithmetic for several selections"""
    from oracle.make_golden import wiring_inputs
    g = load_file(os.path.join(GOLD, "ref_wiring.safetensors"))
    vcfg = C.VAE_TINY
    ecfg = C.emasc_for_vae(vcfg)
    vsd = C.synth_state_dict(C.vae_shapes(vcfg), "vae.")
    inp, gen, sizes = wiring_inputs()
    mom, feats = M.vae_encode(vsd, vcfg, inp["image"])
    assert len(feats) == 6 and torch.equal(feats[0], inp["image"])
    assert torch.allclose(mom, g["enc.moments"], atol=2e-5, rtol=1e-5)
    for i in range(1, 6):
        assert torch.allclose(feats[i][:, :, ::4, ::4], g["enc.feat%d" % i], atol=2e-5, rtol=1e-5), i
        assert torch.allclose(feats[i].double().sum(dim=(2, 3)).float(), g["enc.feat%d.sum" % i], atol=2e-3, rtol=1e-5), i
    noise = torch.randn(mom[:, :4].shape, generator=torch.Generator().manual_seed(7))
    assert torch.allclose(M.posterior_sample(mom, noise), g["enc.sample"], atol=2e-5, rtol=1e-5)
    z = torch.randn((2, 4, 16, 8), generator=gen)
    skips = [torch.randn((2, c, h, w), generator=gen) * 0.5 for c, (h, w) in zip(ecfg["out_channels"], sizes)]
    assert torch.allclose(M.vae_decode(vsd, vcfg, z)[:, :, ::4, ::4], g["dec.plain"], atol=5e-5, rtol=1e-5)
    for name, layers in (("12345", [1, 2, 3, 4, 5]), ("2345", [2, 3, 4, 5]), ("345", [3, 4, 5])):
        lst = [skips[i - 1].clone() for i in layers]
        first = lst[0]
        out = M.vae_decode(vsd, vcfg, z, lst, layers)
        assert lst[-1] is first
        assert torch.allclose(out[:, :, ::4, ::4], g["dec." + name], atol=5e-5, rtol=1e-5), name
    assert not torch.allclose(g["dec.12345"], g["dec.2345"], atol=1e-3)        # the selections really differ


def test_oracle_matches_real_reference_pipeline():
    """fixture = the REAL StableDiffusionTryOnePipeline.__call__ (src/vto_pipelines/tryon_pipe.py:494-765) on the CPU: every UNet input
    it assembled (CFG order [uncond; cond], 31-channel order, zero pose / cloth in the uncond half, cloth zeroing from
    `i >= steps - (1 - rate) * steps` including PNDM's extra evaluation), the prompt batch, the in-place mask binarisation and
    the decoded images; the oracle pipeline must retrace all of it from the same three RNG draws"""
    from oracle.make_golden import WIRING_CASES, WIRING_CASES_LMS, wiring_inputs
    g = load_file(os.path.join(GOLD, "ref_wiring.safetensors"))
    g.update(load_file(os.path.join(GOLD, "ref_wiring_lms.safetensors")))      # LMS: init_noise_sigma / scale_model_input placement
    vcfg, ucfg = C.VAE_TINY, C.UNET_TINY
    ecfg = C.emasc_for_vae(vcfg)
    vsd = C.synth_state_dict(C.vae_shapes(vcfg), "vae.")
    usd = C.synth_state_dict(C.unet_shapes(ucfg), "unet.")
    esd = C.synth_state_dict(C.emasc_shapes(ecfg), "emasc.")
    for name, sched, steps, ccr, gscale, use_emasc, cit, no_pose in WIRING_CASES + WIRING_CASES_LMS:
        inp, _, _ = wiring_inputs()
        calls = []

        def unet_fn(x, t, e):
            calls.append((x.clone(), float(t) if sched == "lms" else int(t), e.clone()))
            return M.unet_forward(usd, ucfg, x, t, e)

        img, _ = P.tryon_pipeline(usd, ucfg, vsd, vcfg, esd if use_emasc else None, inp, num_inference_steps=steps, guidance_scale=gscale,
                                  scheduler=sched, cloth_cond_rate=ccr, no_pose=no_pose, unet_fn=unet_fn)
        ref_in = g["pipe.%s.unet_in" % name].float()
        assert [c[1] for c in calls] == g["pipe.%s.timesteps" % name].tolist(), name
        assert len(calls) == ref_in.shape[0] == (steps + 1 if sched == "pndm" else steps)
        assert torch.equal(calls[0][2], g["pipe.%s.ehs" % name]), name
        got_in = torch.stack([c[0] for c in calls])
        assert got_in.shape == ref_in.shape and got_in.shape[2] == 31
        if sched == "lms":      # the 4 latent channels of evaluation 0 are noise * init_noise_sigma / sqrt(sigma_0^2 + 1), nothing else is scaled
            s0 = 14.614646911621094
            want0 = inp["noise_latents"] * s0 / (s0 * s0 + 1) ** 0.5
            assert torch.allclose(ref_in[0, ref_in.shape[1] // 2:, 0:4], want0.half().float(), atol=2e-3, rtol=2e-3)
            assert any(t != int(t) for t in g["pipe.%s.timesteps" % name].tolist())      # fractional timesteps reach the UNet
        # fixture inputs are stored in fp16: compare at that resolution (relative 1e-3), channel group by channel group
        for lo, hi in ((0, 4), (4, 5), (5, 9), (9, 27), (27, 31)):
            a, b = got_in[:, :, lo:hi], ref_in[:, :, lo:hi]
            assert torch.allclose(a, b, atol=2e-3, rtol=2e-3), (name, lo, float((a - b).abs().max()))
        # structure checks that do not depend on tolerances
        nb = got_in.shape[1] // 2 if gscale > 1 else 0
        if nb:
            assert float(ref_in[:, :nb, 9:31].abs().max()) == 0.0                    # uncond half: zero pose and cloth
        first_zero = next((i for i in range(ref_in.shape[0]) if float(ref_in[i, :, 27:31].abs().max()) == 0.0), None)
        want = next((i for i in range(ref_in.shape[0]) if i >= steps - (1 - ccr) * steps), None)
        assert first_zero == want, (name, first_zero, want)
        assert torch.allclose(img[:, ::2, ::2], g["pipe.%s.images" % name], atol=2e-4), (name, float((img[:, ::2, ::2] - g["pipe.%s.images" % name]).abs().max()))
        m = g["pipe.%s.mask_after" % name]
        assert set(m.unique().tolist()) <= {0.0, 1.0} and float(m[0, 0, 6, 4]) == 0.0 and float(m[0, 0, 62, 31]) == 1.0


def test_oracle_matches_transformers_clip_layer_fixture():
    c = load_file(os.path.join(GOLD, "clip_encoder_layer_tiny.safetensors"))
    sd = C.synth_state_dict(C.adapter_shapes(C.ADAPTER_TINY), "adapter.")
    y = M.clip_encoder_layer(sd, "encoder_layers.0", c["x"], C.ADAPTER_TINY["heads"], C.ADAPTER_TINY["layer_norm_eps"])
    assert torch.allclose(y, c["y"], atol=2e-5, rtol=1e-5)


def test_text_oracle_matches_reference_golden():
    """fixture = the reference's OWN encode_text_word_embedding (src/utils/encode_text_word_embedding.py) run on the installed
    transformers CLIPTextModel (oracle/make_golden.py): '$' splice (first occurrence anchors, num_vstar = 3), rows without '$',
    causal text transformer, final LayerNorm, pooled output at argmax(input_ids)"""
    from oracle import text as T
    c = load_file(os.path.join(GOLD, "clip_text_tiny.safetensors"))
    sd = C.synth_state_dict(C.text_shapes(C.TEXT_TINY), "text.")
    hs, pooled = T.clip_text_forward(sd, C.TEXT_TINY, c["input_ids"], c["word_embeddings"], 3)
    assert torch.allclose(hs, c["last_hidden_state"], atol=3e-5, rtol=1e-5)
    assert torch.allclose(pooled, c["pooler_output"], atol=3e-5, rtol=1e-5)
    assert C.param_count(C.text_shapes(C.TEXT_FULL)) == 340_387_840          # SD2 text encoder (23-layer OpenCLIP ViT-H text tower)
    # splice semantics in isolation: untouched rows, first-'$' anchoring, slots past the sequence end are an error
    ids = c["input_ids"].long()
    emb = torch.zeros((ids.shape[0], ids.shape[1], 4))
    we = torch.arange(ids.shape[0] * 3 * 4, dtype=torch.float32).view(ids.shape[0], 3, 4) + 1
    out = T.splice_word_embeddings(emb, ids, we, 3)
    assert torch.equal(out[0, 10:13], we[0]) and torch.equal(out[2, 5:8], we[2]) and out[2, 30].abs().sum() == 0
    assert out[1].abs().sum() == 0 and out[3].abs().sum() == 0
    bad = ids.clone(); bad[1, 76] = 259
    with pytest.raises(IndexError):
        T.splice_word_embeddings(emb, bad, we, 3)


def test_vision_oracle_matches_transformers_golden():
    """fixture = installed transformers CLIPVisionModel (the third-party class behind src/inference.py:269-273) on the tiny checkpoint"""
    from oracle import vision as V
    c = load_file(os.path.join(GOLD, "clip_vision_tiny.safetensors"))
    sd = C.synth_state_dict(C.vision_shapes(C.VISION_TINY), "vision.")
    hs, pooled = V.clip_vision_forward(sd, C.VISION_TINY, c["pixel_values"])
    assert torch.allclose(hs, c["last_hidden_state"], atol=5e-5, rtol=1e-5)
    assert torch.allclose(pooled, c["pooler_output"], atol=5e-5, rtol=1e-5)
    assert C.param_count(C.vision_shapes(C.VISION_FULL)) == 630_766_080     # ViT-H/14 vision tower without the 1280x1024 projection


def test_warp_oracle_matches_reference_modules_golden():
    """fixture = the REAL reference ConvNet_TPS sub-modules + UNetVanilla (oracle/make_golden.py) on the deterministic checkpoint;
    inputs are regenerated from the seed, only outputs are stored"""
    import warnings
    from oracle import warp as W
    from oracle.make_golden import warp_inputs
    c = load_file(os.path.join(GOLD, "warp_modules.safetensors"))
    tsd = C.synth_state_dict(C.tps_shapes(C.TPS_FULL), "tps.", fp16_round=False)
    tsd["loc_net.regression.linear.weight"] = tsd["loc_net.regression.linear.weight"] * 0.2
    rsd = C.synth_state_dict(C.refine_shapes(C.REFINE_FULL), "refine.", fp16_round=False)
    cloth, agnostic, refine_in = warp_inputs()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fa = W.l2norm(W.feature_extraction(tsd, "extractionA", cloth, 3))
        fb = W.l2norm(W.feature_extraction(tsd, "extractionB", agnostic, 3))
        corr = W.correlation(fa, fb)
        grid, coor = W.tps_forward(tsd, C.TPS_FULL, cloth, agnostic)
        warped = W.warp(cloth, grid)
        refined = W.refinement_forward(rsd, refine_in)
    assert torch.allclose(corr[:, :, ::4, ::4], c["corr_sample"], atol=1e-5, rtol=1e-4)
    assert torch.allclose(coor, c["coor"], atol=1e-5, rtol=1e-4) and coor.abs().max() < 0.999   # tanh not saturated: a real check
    assert torch.allclose(grid, c["grid"].float(), atol=2e-3)                                  # fixture stored as fp16
    assert torch.allclose(warped, c["warped"].float(), atol=5e-3)
    assert torch.allclose(refined, c["refined"], atol=1e-4, rtol=1e-4)
    assert grid.shape == (1, 256, 192, 2) and refined.shape == (1, 3, 64, 48)


@pytest.mark.parametrize("tag,damp", [("", 0.2), ("_raw", 1.0)])
def test_warp_oracle_matches_composed_reference_golden(tag, damp):
    """the COMPOSED warping stage (src/inference.py:239-266: antialiased resizes -> TPS -> grid up-sampling -> border grid_sample -> concat
    -> refinement UNet -> clamp) of the oracle against the fixture made from the REAL reference modules, for the damped (tanh in its linear
    range) and the raw synthetic regression weights"""
    import warnings
    from oracle import warp as W
    from oracle.make_golden import warp_composed_inputs, warp_composed_weights
    c = load_file(os.path.join(GOLD, "warp_composed.safetensors"))
    tsd, rsd = warp_composed_weights(damp)
    cloth, im_mask, pose_map = warp_composed_inputs()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        refined, theta, low_grid, warped = W.warp_cloth(tsd, C.TPS_FULL, rsd, cloth, im_mask, pose_map)
    assert torch.allclose(theta, c["theta" + tag], atol=1e-5, rtol=1e-4)
    assert torch.allclose(low_grid[:, ::4, ::4], c["low_grid_sub" + tag], atol=2e-5)
    assert torch.allclose(warped[:, :, ::4, ::4], c["warped_sub" + tag], atol=1e-4)
    assert torch.allclose(refined, c["refined" + tag].float(), atol=2e-3)            # fixture stored as fp16
    assert refined.shape == (1, 3, 384, 288) and float(refined.abs().max()) <= 1.0
    if damp == 0.2:
        assert theta.abs().max() < 0.999                                              # tanh not saturated: errors upstream are not hidden


def test_mask_features_progressive_equals_strided():
    """the progressive nearest chain equals mask[..., ::s, ::s] (what the native kernels implement)"""
    g = torch.Generator().manual_seed(0)
    mask = (torch.rand((2, 1, 64, 48), generator=g) > 0.5).float()
    feats = [torch.ones(2, 1, 64, 48), torch.ones(2, 1, 64, 48), torch.ones(2, 1, 32, 24), torch.ones(2, 1, 16, 12), torch.ones(2, 1, 8, 6)]
    out = M.mask_features(feats, mask)
    for f, s in zip(out, (1, 1, 2, 4, 8)):
        assert torch.equal(f, 1 - mask[..., ::s, ::s])
    pose = torch.rand((1, 3, 64, 48), generator=g)
    lo = torch.nn.functional.interpolate(pose, size=(8, 6), mode="bilinear")
    ref = 0.25 * (pose[..., 3::8, 3::8] + pose[..., 3::8, 4::8] + pose[..., 4::8, 3::8] + pose[..., 4::8, 4::8])
    assert torch.allclose(lo, ref, atol=1e-6)


def test_oracle_pipeline_smoke_and_cloth_quirk():
    """tiny oracle pipeline runs; PNDM zeroes the cloth latents at the LAST evaluation only (tryon_pipe.py:718-719)"""
    usd = C.synth_state_dict(C.unet_shapes(C.UNET_TINY), "unet.")
    vsd = C.synth_state_dict(C.vae_shapes(C.VAE_TINY), "vae.")
    esd = C.synth_state_dict(C.emasc_shapes(C.EMASC_TINY), "emasc.")
    inp = P.synthetic_inputs(1, 64, 64, L=4, D=C.UNET_TINY["cross_attention_dim"])
    seen = []

    def spy(x, t, e):
        seen.append(float(x[:, 27:31].abs().max()))
        return torch.zeros(x.shape[0], 4, x.shape[2], x.shape[3])

    img, lat = P.tryon_pipeline(usd, C.UNET_TINY, vsd, C.VAE_TINY, esd, inp, num_inference_steps=4, scheduler="pndm", unet_fn=spy)
    assert img.shape == (1, 64, 64, 3) and float(img.min()) >= 0 and float(img.max()) <= 1
    assert len(seen) == 5 and all(v > 0 for v in seen[:4]) and seen[4] == 0.0


# --------------------------------------------------------------------------------------------------------------- C ABI surface
def test_library_loads_and_exports_every_declared_symbol(lib):
    from ladi_vton_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ladi_native.h")).read()
    declared = set(re.findall(r"\b(ladi_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ladi_[a-z0-9_]+)", nm))
    assert declared <= exported, declared - exported
    assert lib.ladi_version() >= 100


def test_igemm_tile_table_names_every_configuration(lib):
    """host side of the GEMM family: every tile configuration 1..ladi_igemm_cfg_count() maps to the kernel symbol rocprofv3 reports for it
    (bench.py groups its roofline by these names; profiles/r03_*), the table has the size the docs quote, and each kernel family is present"""
    n = lib.ladi_igemm_cfg_count()
    assert n == 109
    names = [lib.ladi_igemm_cfg_symbol_name(c).decode() for c in range(1, n + 1)]
    # the X-stationary configurations name their family only: the template arguments depend on the launch (K, LayerNorm, epilogue mode) and
    # are resolved per recorded launch by ladi_profile_igemm_symbols
    assert all(re.fullmatch(r"(igemm_kernel|igemm8_kernel|igemm_lc_kernel|igemm_halo_kernel)<[0-9a-z, ]+>|linear_xs_kernel", s) for s in names), names
    fam = {s.split("<")[0] for s in names}
    assert fam == {"igemm_kernel", "igemm8_kernel", "igemm_lc_kernel", "igemm_halo_kernel", "linear_xs_kernel"}, fam
    assert names[84 - 1] == "igemm_halo_kernel<2, 2, 1, 2, 2, 48, 0, 0, 0>"    # the dominant symbol of the round-3 forward (profiles/r03_bench_default.json)
    assert names[92 - 1] == "igemm_halo_kernel<5, 1, 1, 2, 6, 48, 0, 0, 0>"    # round 4: the 12-wave 320x192 form (256 workgroups on the 64x48 level)
    # round 6: halo symbols carry EVERY template argument, as rocprofv3 prints them, so that a ring-halo form and the 2-D blocked form of the same
    # leading arguments (cfg 75 / 101) can never be taken for each other when bench.py looks a symbol up in a committed trace
    assert names[75 - 1] == "igemm_halo_kernel<4, 2, 1, 3, 4, 48, 0, 0, 0>" and names[101 - 1] == "igemm_halo_kernel<4, 2, 1, 3, 4, 48, 0, 1, 0>"
    assert names[105 - 1] == "igemm_halo_kernel<5, 1, 1, 2, 6, 48, 0, 0, 1>"      # round 6: the folded-upsample forms (UPS = 1)
    # every name, byte for byte: bench.py looks these strings up in committed traces, and tune tables store the ids they belong to
    with open(os.path.join(ROOT, "tests", "golden", "igemm_cfg_symbols.txt")) as fh:
        golden = fh.read().split("\n")[:-1]
    assert names == golden, [(c + 1, a, b) for c, (a, b) in enumerate(zip(names, golden)) if a != b]
    assert not lib.ladi_igemm_cfg_symbol_name(0) and not lib.ladi_igemm_cfg_symbol_name(n + 1)   # out of range: empty, not a crash


def test_bench_d2h_pil_tail_encodes_every_image():
    """the `with_d2h_pil_images_per_s` leg of bench.py: one JPEG (quality 95) per sample of the uint8 batch, as inference.py:314-324 saves them;
    the byte count it returns is the sum over the batch and the images decode back to the input size"""
    import io
    import bench
    from PIL import Image
    g = torch.Generator().manual_seed(3)
    batch = (torch.rand((3, 64, 48, 3), generator=g) * 255).to(torch.uint8)
    n = bench.d2h_pil_tail(batch)
    sizes = []
    for im in batch.numpy():
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=95)
        sizes.append(buf.tell())
        assert Image.open(io.BytesIO(buf.getvalue())).size == (48, 64)
    assert n == sum(sizes) and all(s > 0 for s in sizes)


def test_native_host_scheduler_tables_match_oracle(lib):
    buf = (ctypes.c_int * 1100)()
    for kind in (0, 1):
        for n in (7, 20, 50, 100):
            cnt = lib.ladi_sched_timesteps(kind, n, buf, 1100)
            sch = P.make_scheduler(kind); sch.set_timesteps(n)
            assert list(buf[:cnt]) == sch.timesteps
    out = (ctypes.c_float * 1000)()
    assert lib.ladi_sched_alphas_cumprod(out) == 0
    ac = P.alphas_cumprod()
    got = torch.tensor(list(out))
    assert float(((got - ac).abs() / ac).max()) < 5e-6


def test_lms_scheduler_tables_and_host_step_match_oracle(lib):
    """LMSDiscreteScheduler (the third scheduler tryon_pipe.py:62 accepts): native table builder (closed-form Gauss-Legendre integrals of
    the Lagrange basis) vs the oracle's restatement of diffusers 0.14 (scipy quad, epsrel 1e-4); known-answer anchors of the algorithm:
    init_noise_sigma = 14.6146 for the SD beta schedule, sum_j c_ij = sigma_{i+1} - sigma_i (the basis polynomials sum to 1), first step
    = one Euler step; then the host-side shim's scale_model_input / step vs the oracle on a random trajectory"""
    import ladi_vton_amd as L
    for n in (5, 20, 50):
        ts, sg, cf = (ctypes.c_double * n)(), (ctypes.c_float * (n + 1))(), (ctypes.c_float * (4 * n))()
        ac = P.alphas_cumprod().contiguous()
        assert lib.ladi_sched_lms(n, ctypes.c_void_p(ac.data_ptr()), ts, sg, cf) == n
        o = P.make_scheduler("lms"); o.set_timesteps(n)
        assert list(ts) == o.timesteps                                         # float64 linspace, bit-equal
        assert np.allclose(np.array(list(sg)), o.sigmas, rtol=2e-6, atol=0)
        assert abs(sg[0] - 14.6146) < 1e-3 and sg[n] == 0.0
        co = np.array(list(cf)).reshape(n, 4)
        for i in range(n):
            order = min(i + 1, 4)
            want = [o.coefficient(order, i, j) for j in range(order)]
            assert np.allclose(co[i, :order], want, rtol=2e-4, atol=2e-6), (n, i)
            assert not co[i, order:].any()
            assert abs(co[i].sum() - (o.sigmas[i + 1] - o.sigmas[i])) < 1e-4 * abs(o.sigmas[i])
        assert abs(co[0, 0] - (o.sigmas[1] - o.sigmas[0])) < 1e-5 * abs(o.sigmas[0])        # Euler
    with pytest.raises(Exception):
        buf = (ctypes.c_int * 64)()
        assert lib.ladi_sched_timesteps(2, 20, buf, 64) >= 0                  # fractional timesteps have their own entry point
    n = 12
    s, o = L.LMSDiscreteScheduler(), P.make_scheduler("lms")
    assert abs(s.init_noise_sigma - 14.6146) < 1e-3                            # available before set_timesteps, as in diffusers
    s.set_timesteps(n); o.set_timesteps(n)
    assert s.timesteps.dtype == torch.float64 and s.timesteps.tolist() == o.timesteps
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 8, 6), generator=g) * s.init_noise_sigma
    xo = x.clone()
    for t in s.timesteps:
        assert torch.allclose(s.scale_model_input(x, t), o.scale_model_input(xo, float(t)), rtol=1e-5, atol=1e-6)
        e = torch.randn((2, 4, 8, 6), generator=g)
        x, xo = s.step(e, t, x).prev_sample, o.step(e, float(t), xo)
        assert torch.allclose(x, xo, rtol=1e-4, atol=1e-4)
    with pytest.raises(NotImplementedError):
        s.step(e, s.timesteps[0], x, order=2)


def test_no_cpu_fallback():
    import ladi_vton_amd as L
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.NativeError):
        L.NativeUNet(C.UNET_TINY, {})
    with pytest.raises(L.NativeError):
        L.build_random_init_pipeline("tiny")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "ladi_vton_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "/root/reference" not in src, f


# --------------------------------------------------------------------------------------------------------------- host logic
def test_shim_schedulers_match_oracle_on_cpu():
    import ladi_vton_amd as L
    g = torch.Generator().manual_seed(3)
    for kind, cls in ((0, L.DDIMScheduler), (1, L.PNDMScheduler)):
        s, o = cls(), P.make_scheduler(kind)
        s.set_timesteps(9); o.set_timesteps(9)
        assert [int(t) for t in s.timesteps] == o.timesteps
        x = torch.randn((2, 4, 8, 6), generator=g)
        xs, xo = x.clone(), x.clone()
        for t in o.timesteps:
            e = torch.randn((2, 4, 8, 6), generator=g)
            xs = s.step(e, t, xs).prev_sample
            xo = o.step(e, t, xo)
        assert torch.allclose(xs, xo, rtol=1e-5, atol=1e-5)
        assert s.init_noise_sigma == 1.0 and s.order == 1 and s.config.steps_offset == 1 and s.config.skip_prk_steps is True
        assert s.scale_model_input(x, 5) is x
    # DDIM with eta > 0 (tryon_pipe.py:331-346 passes eta / generator through to scheduler.step): the stochastic term, drawn from the
    # generator exactly once per step with the sample's shape, vs the oracle's eq. (12) with the same draws
    s, o = L.DDIMScheduler(), P.make_scheduler(0)
    s.set_timesteps(7); o.set_timesteps(7)
    x = torch.randn((2, 4, 8, 6), generator=g)
    xs, xo = x.clone(), x.clone()
    gs, go = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    for t in o.timesteps:
        e = torch.randn((2, 4, 8, 6), generator=g)
        xs = s.step(e, t, xs, eta=0.7, generator=gs).prev_sample
        xo = o.step(e, t, xo, eta=0.7, noise=torch.randn((2, 4, 8, 6), generator=go))
    assert torch.allclose(xs, xo, rtol=1e-5, atol=1e-5)


def test_pipeline_generator_lists_draw_per_sample():
    """diffusers randn_tensor semantics for a list of generators (tryon_pipe.py:443-455): sample i of every draw comes from generator i"""
    import ladi_vton_amd as L
    pipe = L.StableDiffusionTryOnePipeline.__new__(L.StableDiffusionTryOnePipeline)
    gens = [torch.Generator().manual_seed(5 + i) for i in range(3)]
    a = pipe._draw((3, 4, 2, 2), gens, torch.float32, torch.device("cpu"))
    b = pipe._draw((3, 4, 2, 2), gens, torch.float32, torch.device("cpu"))
    for i in range(3):
        gi = torch.Generator().manual_seed(5 + i)
        assert torch.equal(a[i], torch.randn((1, 4, 2, 2), generator=gi)[0]) and torch.equal(b[i], torch.randn((1, 4, 2, 2), generator=gi)[0])
    with pytest.raises(ValueError):
        pipe._draw((2, 4, 2, 2), gens, torch.float32, torch.device("cpu"))


def test_pipeline_check_inputs_errors():
    """same ValueErrors as tryon_pipe.py:362-407"""
    import ladi_vton_amd as L
    from types import SimpleNamespace
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    pipe = L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=SimpleNamespace(), scheduler=L.DDIMScheduler())
    assert pipe.vae_scale_factor == 8
    pe = torch.zeros(1, 77, 8)
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 510, 384, 1, prompt_embeds=pe)
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 512, 384, 0, prompt_embeds=pe)
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 512, 384, 1, prompt_embeds=pe)
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 512, 384, 1)
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 512, 384, 1, prompt_embeds=pe, negative_prompt_embeds=torch.zeros(2, 77, 8))
    pipe.check_inputs(None, 512, 384, 1, prompt_embeds=pe, negative_prompt_embeds=pe)
    with pytest.raises(ValueError):
        L.StableDiffusionTryOnePipeline._validate_images(torch.full((1, 3, 8, 8), 2.0), torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError):
        L.StableDiffusionTryOnePipeline._validate_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 4, 8))


def test_on_disk_formats_roundtrip_with_reference_readers(tmp_path):
    """files written by ladi_vton_amd.io must be readable with the exact calls the reference uses (vitonhd.py:100-107,
    inference.py:314-324) and vice versa"""
    import pickle
    from ladi_vton_amd import io as IO
    from ladi_vton_amd.pipeline import numpy_to_pil
    root = str(tmp_path)
    feats = torch.randn((3, 257, 16))
    names = ["00001_00.jpg", "00002_00.jpg", "00003_00.jpg"]
    ft, nm = IO.save_clip_cloth_features(root, "vitonhd", "test", feats, names)
    assert ft.endswith("data/clip_cloth_embeddings/vitonhd/test_last_hidden_state_features.pt") and nm.endswith("test_features_names.pkl")
    raw = torch.load(ft, map_location="cpu")                       # the reference's reader
    with open(nm, "rb") as f:
        raw_names = pickle.load(f)
    assert raw.dtype == torch.float16 and raw.shape == (3, 257, 16) and raw_names == names
    got, got_names = IO.load_clip_cloth_features(root, "vitonhd", "test")
    assert torch.equal(got, feats.half()) and got_names == names and not got.requires_grad
    assert torch.equal(got[got_names.index("00002_00.jpg")], feats[1].half())
    with pytest.raises(ValueError):
        IO.save_clip_cloth_features(root, "vitonhd", "bad", feats, names[:2])
    # checkpoints: plain state_dict and the {'tps', 'refinement'} container of the warping release
    sd = {"conv.weight": torch.randn(2, 2), "conv.bias": torch.zeros(2)}
    torch.save(sd, os.path.join(root, "emasc_vitonhd.pth"))
    torch.save({"tps": sd, "refinement": sd}, os.path.join(root, "warping_vitonhd.pth"))
    assert torch.equal(IO.load_released_state_dict(os.path.join(root, "emasc_vitonhd.pth"))["conv.weight"], sd["conv.weight"])
    assert set(IO.load_released_state_dict(os.path.join(root, "warping_vitonhd.pth"), "tps")) == set(sd)
    with pytest.raises(ValueError):
        IO.load_released_state_dict(os.path.join(root, "warping_vitonhd.pth"))
    # images: {save_dir}/{category}/{name}, JPEG q95 or PNG with the .jpg -> .png rename
    from PIL import Image
    imgs = numpy_to_pil(torch.rand((2, 16, 12, 3)).numpy())
    paths = IO.save_generated_images(imgs, os.path.join(root, "out"), ["upper_body", "dresses"], ["a.jpg", "b.jpg"], use_png=False)
    assert [os.path.relpath(p, root) for p in paths] == ["out/upper_body/a.jpg", "out/dresses/b.jpg"]
    assert Image.open(paths[0]).format == "JPEG" and Image.open(paths[0]).size == (12, 16)
    paths = IO.save_generated_images(imgs, os.path.join(root, "out"), ["upper_body", "dresses"], ["a.jpg", "b.jpg"], use_png=True)
    assert paths[1].endswith("out/dresses/b.png") and Image.open(paths[1]).format == "PNG"


def test_shard_bounds_cover_batch():
    from ladi_vton_amd.parallel import shard_bounds
    for B in (1, 7, 8, 32, 255, 256):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(B, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == B
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
from ladi_vton_amd.parallel import run_sharded, shard_bounds
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[3]
dist.init_process_group("gloo", rank=rank, world_size=world)
B = 5   # ragged over 2 ranks
g = torch.Generator().manual_seed(7)
inputs = dict(image=torch.rand((B, 3, 8, 6), generator=g), noise=torch.rand((B, 4, 1, 1), generator=g), scalar=3)
def run_local(loc):   # stand-in for the per-rank pipeline: a per-sample function of the sharded inputs
    assert loc["scalar"] == 3
    return (loc["image"] * loc["noise"][:, :3]).permute(0, 2, 3, 1).contiguous()
out = run_sharded(run_local, inputs)
ref = ((inputs["image"] * inputs["noise"][:, :3]).permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8)
assert out.shape == ref.shape and torch.equal(out, ref), (rank, out.shape)
# the row-materialiser form (what bench.py uses: a rank only ever builds its own rows of the global batch) gives the same batch
seen = []
def rows(lo, hi):
    seen.append((lo, hi))
    return {k: (v[lo:hi] if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}
out2 = run_sharded(run_local, rows, batch=B)
assert torch.equal(out2, ref) and seen == [shard_bounds(B, rank, world)], (rank, seen)
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
"""


def test_sharded_run_world_size_2_gloo(tmp_path):
    """N > 1 path on CPU: batch sharding + the all-gather of uint8 images, world_size 2, gloo, ragged batch"""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    port = str(29500 + (os.getpid() % 500))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("OK %d" % r) in o, o


_BENCH_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
import bench
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[3]
dist.init_process_group("gloo", rank=rank, world_size=world)
cfg = bench.CONFIGS[3]                                   # BASELINE configs[3]: 32 pairs per GPU (weak scaling), producers in the step
B, H, W = cfg["batch"], 32, 24                           # real per-GPU batch, small images: this rehearses the WIRING, not the kernels
assert B == 32 and cfg["producers"]
global_B, lo = B * world, rank * B
local = bench.make_rows(lo, lo + B, H, W, 77, 16, "cpu")
def run_local(inp):                                      # stand-in for producers + fused try-on: a per-row function of the row's tensors
    assert inp["image"].shape[0] == B and inp["word_ids"].shape == (B, 77) and inp["prompt_embeds"].shape[0] == B
    x = inp["image"] * 0.25 + inp["cloth"] * 0.25 + 0.5 + inp["noise_latents"].mean(dim=(1, 2, 3)).view(-1, 1, 1, 1) * 0.01
    return x.permute(0, 2, 3, 1).clamp(0, 1).float().contiguous()
step = bench.make_step(run_local, local, lo, B, global_B)
out = step()
assert out.shape == (global_B, H, W, 3) and out.dtype == torch.uint8
# every rank must hold the whole batch, row g a function of g only: rebuild ALL rows here and compare
allrows = bench.make_rows(0, global_B, H, W, 77, 16, "cpu")
parts = []
for r in range(world):
    blk = {k: (v[r * B:(r + 1) * B] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == global_B else v) for k, v in allrows.items()}
    parts.append((run_local(blk) * 255.0).round().clamp(0, 255).to(torch.uint8))
assert torch.equal(out, torch.cat(parts)), rank
n = bench.d2h_pil_tail(out[:2])                          # the output tail of the bench line runs on this host too
assert n > 0
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
"""


def test_bench_step_wiring_config3_world_size_2_gloo(tmp_path):
    """rehearsal of `bench.py --config 3 --gpus N` without a node: bench.make_rows (per-global-row generators),
    bench.make_step (row materialiser -> run_sharded -> all-gather of uint8 images) at the real per-GPU batch of 32 with a stub in
    place of the native pipeline, 2 gloo processes: every rank ends up with the same 64-image batch, row g depending on g only"""
    script = tmp_path / "bench_worker.py"
    script.write_text(_BENCH_WORKER % {"root": ROOT})
    port = str(29000 + (os.getpid() % 400))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("OK %d" % r) in o, o


def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus N` with no launcher around it must START N ranks (it re-executes itself under
    torch.distributed.run, one process per GPU) -- never run one rank and print n_gpus 1.  Driven here with --stub-step (CPU stand-in
    compute, gloo): the launch, WORLD_SIZE check, shard bounds, all-gather, barrier / MAX timing and the printed line are bench.py's own."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--stub-step", "--steps", "2", "--warmup", "1", "--batch", "3",
                        "--height", "32", "--width", "24"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["rccl_ranks_seen"] == 2 and line["config"]["global_batch"] == 6
    assert line["config"]["collective_backend"] == "gloo" and line["data"].startswith("stub")      # cannot be mistaken for a measurement
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["scaling"] == "weak"
    assert "dp2" in line["config"]["parallelism"]


def test_bench_refuses_to_run_fewer_ranks_than_gpus_flag():
    """the two ways the line could contradict the command line: --gpus N on a box with fewer GPUs (here: none), and a launcher that
    started another number of ranks than --gpus says -- both exit non-zero with a message and print no JSON line"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 2 and "--gpus 2" in r.stderr and "{" not in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--stub-step"], capture_output=True, text=True, timeout=300,
                       env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr and "{" not in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_bench_full_option_gates_the_extra_legs(monkeypatch):
    """a plain `bench.py` run carries no leg beyond its timed steps: parse() switches the tail, roofline and CPU-baseline legs off
    unless --full is given, --full keeps the --no-* switches working, and the roofline runs of their own are refused without --full"""
    import bench

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
        return bench.parse()
    a = parse("--gpus", "1", "--steps", "3", "--warmup", "2")
    assert not a.full and a.no_tail and a.no_roofline and a.no_cpu_baseline and (a.steps, a.warmup) == (3, 2)
    a = parse("--gpus", "1", "--steps", "3", "--warmup", "2", "--full")
    assert a.full and not (a.no_tail or a.no_roofline or a.no_cpu_baseline) and (a.steps, a.warmup) == (3, 2)
    a = parse("--full", "--no-cpu-baseline", "--roofline-only")
    assert a.no_cpu_baseline and a.roofline_only and not a.no_roofline
    for flag in ("--roofline-only", "--measure-traffic"):
        with pytest.raises(SystemExit) as e:
            parse(flag)
        assert e.value.code == 2


def test_bench_dump_outputs_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the last timed step returned (DIR/images.npy, float32) and the same arguments give the
    same arrays; an output over the byte budget is reduced to a seeded sample with its flat indices, the same sample every time."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    got = []
    for i, steps in enumerate((2, 3)):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stub-step", "--steps", str(steps), "--warmup", "1",
                            "--batch", "3", "--height", "32", "--width", "24", "--dump-outputs", str(d)], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] is not None and line["ms_per_step"] >= 0
        got.append(np.load(d / "images.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (3, 32, 24, 3) and np.array_equal(got[0], got[1])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stub-step", "--steps", "0",
                        "--dump-outputs", str(tmp_path / "none")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    import bench
    x = torch.arange(60000, dtype=torch.int32).reshape(6, 100, 100)
    budget = 2 * 4096 + 60000
    for d in ("s0", "s1"):
        bench.dump_outputs(str(tmp_path / d), {"images": x}, budget=budget)
    v, idx = np.load(tmp_path / "s0" / "images.npy"), np.load(tmp_path / "s0" / "images_index.npy")
    assert v.dtype == np.float32 and idx.dtype == np.float64 and 0 < v.size < x.numel()
    assert sum(os.path.getsize(tmp_path / "s0" / f) for f in os.listdir(tmp_path / "s0")) <= budget
    assert np.array_equal(v, x.reshape(-1).numpy()[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(tmp_path / "s1" / "images_index.npy"))


def test_dataset_preprocessing_matches_real_reference_classes(tmp_path):
    """ladi_vton_amd.dataset (host-side VITON-HD / DressCode readers: label-map algebra, PIL rasterisation, box dilation, pose heat-maps)
    vs fixtures produced by the REAL src/dataset/vitonhd.py / dresscode.py classes on the same synthetic trees (oracle/make_golden.py:
    make_dataset_golden).  Integer / byte outputs bit-exact; the fp32 maps to 1e-6."""
    from oracle.make_golden import DATASET_KEYS
    from tests import util_data as UD
    from ladi_vton_amd.dataset import DressCodeDataset, VitonHDDataset, dilate_box
    g = load_file(os.path.join(GOLD, "dataset_ref.safetensors"))
    UD.make_vitonhd(str(tmp_path / "viton"), n=4)
    UD.make_dresscode(str(tmp_path / "dc"), per_category=2)
    keys = DATASET_KEYS + ("c_name", "im_name", "category")
    sets = {"viton_unpaired": VitonHDDataset(str(tmp_path / "viton"), "test", order="unpaired", outputlist=keys, size=(128, 96)),
            "dc_paired": DressCodeDataset(str(tmp_path / "dc"), "test", order="paired", outputlist=keys, size=(128, 96))}
    for tag, ds in sets.items():
        assert len(ds) == int(g["%s.len" % tag][0]) and len(ds) >= 4
        for i in range(len(ds)):
            it = ds[i]
            assert bytes(g["%s.%d.names" % (tag, i)].tolist()).decode() == it["im_name"] + "|" + it["c_name"] + "|" + it["category"]
            for k in ("inpaint_mask", "parse_mask_total"):
                assert torch.equal(torch.as_tensor(it[k]).to(torch.uint8), g["%s.%d.%s" % (tag, i, k)]), (tag, i, k)
            assert it["inpaint_mask"].shape == (1, 128, 96) and it["inpaint_mask"].dtype == torch.uint8
            assert 0 < int(it["inpaint_mask"].sum()) < 128 * 96              # the synthetic person really has a garment region
            for k in ("image", "cloth", "im_mask"):
                assert torch.equal(it[k][:, ::2, ::2], g["%s.%d.%s" % (tag, i, k)]), (tag, i, k)
            assert torch.allclose(it["pose_map"][:, ::4, ::4], g["%s.%d.pose_map" % (tag, i)], atol=1e-6, rtol=0)
            assert torch.allclose(it["pose_map"].double().sum(dim=(1, 2)).float(), g["%s.%d.pose_map.sum" % (tag, i)], rtol=1e-6)
            assert it["pose_map"].shape == (18, 128, 96) and float(it["pose_map"][17].abs().max()) == 0.0   # undetected joint
    # the numpy box dilation == cv2.dilate(5x5, iterations=5) as restated by scipy's grey dilation
    from scipy import ndimage
    import numpy as np
    m = (np.random.default_rng(0).random((40, 30)) > 0.97).astype(np.float32) * 255
    ref = m
    for _ in range(5):
        ref = ndimage.grey_dilation(ref, footprint=np.ones((5, 5), bool), mode="constant", cval=0)
    assert np.array_equal(dilate_box(m, 5, 5), ref)
    with pytest.raises(ValueError):
        VitonHDDataset(str(tmp_path / "viton"), "test", outputlist=("dense_uv",))


# ---------------------------------------------------------------------------------------------------------------
# Second source for the arithmetic no reference-held vector pins: the diffusers blocks rebuilt from STOCK torch.nn
# modules (nn.GroupNorm / nn.Conv2d / nn.LayerNorm / nn.MultiheadAttention with kdim / vdim) loaded from the App. A.6 key list, and the
# scheduler recurrences checked against their papers' closed forms.  Two independent derivations instead of one restatement; this does
# not lift the "parity unpinned" cap (neither is reference-held), it shrinks the room for a shared misreading.
# ---------------------------------------------------------------------------------------------------------------
class _NNResnet(torch.nn.Module):
    """ResnetBlock2D from stock modules: norm1 -> SiLU -> conv1 (+ time_emb_proj(SiLU(temb))) -> norm2 -> SiLU -> conv2, + shortcut"""

    def __init__(self, cin, cout, temb, groups, eps):
        super().__init__()
        nn = torch.nn
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=eps), nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb, cout) if temb else None
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=eps), nn.Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None
        self.act = nn.SiLU()

    def forward(self, x, temb):
        h = self.conv1(self.act(self.norm1(x)))
        if self.time_emb_proj is not None:
            h = h + self.time_emb_proj(self.act(temb))[:, :, None, None]
        h = self.conv2(self.act(self.norm2(h)))
        return (self.conv_shortcut(x) if self.conv_shortcut is not None else x) + h


def _mha_from(sd, p, C, heads, kdim=None, bias_qkv=False, out="to_out.0", names=("to_q", "to_k", "to_v")):
    """nn.MultiheadAttention carrying the diffusers attention weights `p`.{to_q,to_k,to_v,to_out.0} (q scaled by head_dim^-0.5 inside)"""
    m = torch.nn.MultiheadAttention(C, heads, bias=True, batch_first=True, kdim=kdim, vdim=kdim)
    wq, wk, wv = (sd[p + "." + n + ".weight"] for n in names)
    with torch.no_grad():
        if kdim is None or kdim == C:
            m.in_proj_weight.copy_(torch.cat([wq, wk, wv]))
        else:
            m.q_proj_weight.copy_(wq); m.k_proj_weight.copy_(wk); m.v_proj_weight.copy_(wv)
        if bias_qkv:
            m.in_proj_bias.copy_(torch.cat([sd[p + "." + n + ".bias"] for n in names]))
        else:
            m.in_proj_bias.zero_()
        m.out_proj.weight.copy_(sd[p + "." + out + ".weight"]); m.out_proj.bias.copy_(sd[p + "." + out + ".bias"])
    return m.eval()


def test_oracle_blocks_match_torch_nn_modules():
    from oracle import models as M
    nn = torch.nn
    g = torch.Generator().manual_seed(3)
    C0, C1, temb_dim, groups, heads, cross, n, h, w, L = 64, 128, 256, 32, 2, 96, 2, 8, 6, 7
    # ---- ResnetBlock2D with a channel change (conv_shortcut) and a time embedding
    shapes = OrderedDict()
    LC._resnet(shapes, "r", C0, C1, temb_dim)
    sd = C.synth_state_dict(shapes, "second.")
    blk = _NNResnet(C0, C1, temb_dim, groups, 1e-5).eval()
    blk.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=True)
    x = torch.randn((n, C0, h, w), generator=g)
    temb = torch.randn((n, temb_dim), generator=g)
    with torch.no_grad():
        want = blk(x, temb)
    got = M.resnet(sd, "r", x, temb, groups, 1e-5)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), float((got - want).abs().max())
    # ---- Transformer2DModel + BasicTransformerBlock (self-attention, cross-attention on `cross`-wide context, GEGLU)
    shapes = OrderedDict()
    LC._transformer(shapes, "t", C1, cross)
    sd = C.synth_state_dict(shapes, "second.")
    b = "t.transformer_blocks.0"
    gn, proj_in, proj_out = nn.GroupNorm(groups, C1, eps=1e-6), nn.Linear(C1, C1), nn.Linear(C1, C1)
    ln = [nn.LayerNorm(C1) for _ in range(3)]
    ff1, ff2, gelu = nn.Linear(C1, 8 * C1), nn.Linear(4 * C1, C1), nn.GELU()
    for mod, key in ((gn, "t.norm"), (proj_in, "t.proj_in"), (proj_out, "t.proj_out"), (ln[0], b + ".norm1"), (ln[1], b + ".norm2"),
                     (ln[2], b + ".norm3"), (ff1, b + ".ff.net.0.proj"), (ff2, b + ".ff.net.2")):
        mod.load_state_dict({"weight": sd[key + ".weight"], "bias": sd[key + ".bias"]}, strict=True)
    attn1 = _mha_from(sd, b + ".attn1", C1, heads)
    attn2 = _mha_from(sd, b + ".attn2", C1, heads, kdim=cross)
    x = torch.randn((n, C1, h, w), generator=g)
    ehs = torch.randn((n, L, cross), generator=g)
    with torch.no_grad():
        t = proj_in(gn(x).permute(0, 2, 3, 1).reshape(n, h * w, C1))
        a = ln[0](t); t = attn1(a, a, a, need_weights=False)[0] + t
        a = ln[1](t); t = attn2(a, ehs, ehs, need_weights=False)[0] + t
        u, gate = ff1(ln[2](t)).chunk(2, dim=-1)
        t = ff2(u * gelu(gate)) + t
        want = proj_out(t).reshape(n, h, w, C1).permute(0, 3, 1, 2) + x
    got = M.transformer2d(sd, "t", x, ehs, heads, groups)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())
    # ---- VAE AttentionBlock (one head of width C, biased q / k / v, residual)
    shapes = OrderedDict()
    LC._vae_attn(shapes, "a", C1)
    sd = C.synth_state_dict(shapes, "second.")
    vgn = nn.GroupNorm(groups, C1, eps=1e-6)
    vgn.load_state_dict({"weight": sd["a.group_norm.weight"], "bias": sd["a.group_norm.bias"]})
    mha = _mha_from(sd, "a", C1, 1, bias_qkv=True, out="proj_attn", names=("query", "key", "value"))
    with torch.no_grad():
        tok = vgn(x).reshape(n, C1, h * w).transpose(1, 2)
        want = mha(tok, tok, tok, need_weights=False)[0].transpose(1, 2).reshape(n, C1, h, w) + x
    got = M.vae_attention(sd, "a", x, groups)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())


def _closed_form(ac, a, x0, e):
    return a ** 0.5 * x0 + (1 - a) ** 0.5 * e


@pytest.mark.parametrize("steps", [50, 20])
def test_scheduler_exact_on_analytic_eps(steps):
    """(1) A model that returns the TRUE noise e of x_t = sqrt(a_t) x0 + sqrt(1 - a_t) e makes every deterministic DDIM step land on the same
    closed form at t - ratio (DDIM eq. 12), and PNDM's transfer formula (eq. 9) is that step rationalised, with linear-multistep weights
    that sum to 1: both schedulers must end exactly at sqrt(a_final) x0 + sqrt(1 - a_final) e, a_final = alphas_cumprod[0]
    (set_alpha_to_one = False).  Checked for the oracle classes and for the product's host schedulers.
    (2) On a noise prediction that is LINEAR in t, the 4th-order Adams-Bashforth combination (55, -59, 37, -9) / 24 over equally spaced
    evaluations equals the prediction at the step's midpoint t - ratio / 2, and the warm-up orders (1, 3/2 -1/2, 23/12 -16/12 5/12) equal
    it at t, t - ratio / 2, t - ratio / 2: the effective epsilon recovered from each PLMS step must match."""
    from oracle import pipeline as P
    import ladi_vton_amd.schedulers as S
    g = torch.Generator().manual_seed(steps)
    x0 = torch.randn((1, 4, 8, 6), generator=g, dtype=torch.float64)
    e = torch.randn((1, 4, 8, 6), generator=g, dtype=torch.float64)
    ac = P.alphas_cumprod().double()
    want = _closed_form(ac, ac[0], x0, e)
    for kind in ("ddim", "pndm"):
        sch = P.make_scheduler(kind)
        sch.set_timesteps(steps)
        sch.ac = sch.ac.double(); sch.final_ac = sch.ac[0]
        x = _closed_form(ac, ac[sch.timesteps[0]], x0, e)
        for t in sch.timesteps:
            x = sch.step(e, t, x)
        assert torch.allclose(x, want, rtol=0, atol=1e-9), (kind, float((x - want).abs().max()))
        prod = S.DDIMScheduler() if kind == "ddim" else S.PNDMScheduler()
        prod.set_timesteps(steps)
        xp = _closed_form(ac, ac[int(prod.timesteps[0])], x0, e).float()
        for t in prod.timesteps:
            xp = prod.step(e.float(), t, xp).prev_sample
        assert torch.allclose(xp.double(), want, rtol=0, atol=2e-4), (kind, float((xp.double() - want).abs().max()))
    # (2) effective epsilon of each PLMS step on eps(t) = e0 + t * e1
    e1 = torch.randn((1, 4, 8, 6), generator=g, dtype=torch.float64) * 1e-3
    sch = P.make_scheduler("pndm")
    sch.set_timesteps(steps)
    sch.ac = sch.ac.double(); sch.final_ac = sch.ac[0]
    ratio = 1000 // steps
    x = torch.randn((1, 4, 8, 6), generator=g, dtype=torch.float64)
    for i, t in enumerate(sch.timesteps):
        eps_t = e + t * e1
        cur = sch.cur_sample if i == 1 else x
        xn = sch.step(eps_t, t, x)
        # invert the transfer formula (PNDM eq. 9) for the epsilon the step used
        t_from, t_to = (t + ratio, t) if i == 1 else (t, t - ratio)
        a_t, a_p = ac[t_from], (ac[t_to] if t_to >= 0 else ac[0])
        coeff = (a_p / a_t) ** 0.5
        denom = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
        used = (coeff * cur - xn) * denom / (a_p - a_t)
        if i == 0:
            mid = float(t)                       # first evaluation: plain step with eps(t)
        elif i == 1:
            mid = t + ratio / 2.0                # second evaluation: (eps(t) + eps(t + ratio)) / 2 from the saved sample
        else:
            mid = t - ratio / 2.0                # orders 2, 3 and 4 all extrapolate a linear function to the step's midpoint
        assert torch.allclose(used, e + mid * e1, rtol=0, atol=1e-8), (i, t, float((used - (e + mid * e1)).abs().max()))
        x = xn


def test_bench_hbm_kernels_reads_the_committed_profiles(monkeypatch):
    """`roofline.hbm_kernels` / `roofline.traffic` of bench.py: GB/s = (2 x FETCH_SIZE + WRITE_SIZE) of the committed PMC passes / the average
    duration of the committed kernel trace, accepted only for the library digest stamped into the files' first line"""
    import bench
    path = os.path.join(ROOT, "profiles", "%s_pmc_fetch_size.txt" % bench.PROFILE_ROUND)
    if not os.path.exists(path):
        pytest.skip("the PMC passes of %s are not committed yet" % bench.PROFILE_ROUND)
    dig = re.match(r"# lib_digest=(\w+)", open(path).readline()).group(1)
    monkeypatch.setattr(bench, "lib_digest", lambda: dig)
    h = bench.hbm_kernels()
    ga = h["unet_forward"]["gn_norm_kernel"]          # round 5: the UNet's GroupNorms are one-pass launches (finalize folded into apply)
    assert 500.0 < ga["GBps"] < 8000.0 and abs(ga["GBps"] - ga["MB_per_launch"] * 1e3 / ga["avg_us"]) < 1.0, ga
    assert any("gn_" in k for k in h["vae_stages"]) and "source" in h      # (round 6: the VAE's GroupNorms are gn_reduce_rows + gn_norm launches)
    t, why = bench.traffic_committed("igemm_halo_kernel<2, 2, 1, 3, 2, 24, 0, 0, 0>")
    assert why is None and abs(t["bytes_per_launch"] - (t["fetch_bytes_x2"] + t["write_bytes"])) <= 2 and t["bytes_per_launch"] > 10_000_000   # each term is rounded on its own
    monkeypatch.setattr(bench, "lib_digest", lambda: "another-build")
    t, why = bench.traffic_committed("igemm_halo_kernel<2, 2, 1, 3, 2, 24, 0, 0, 0>")
    assert t is None and "stale" in why
    assert "note" in bench.hbm_kernels()["unet_forward"]


def test_fragment_chain_emulations_of_the_fused_prototypes():
    """tools/experiments/next: the stand-alone fused-block prototypes (xattn_q / xattn_full / ff_fused) rest on one identity -- a 32x32 MFMA
    accumulator block is the B operand of the next product once the A side reads its rows as two 8-byte pieces -- and on a page of index
    arithmetic (LDS-DMA swizzle, packed K / V^T / Wo / W2 tiles, ring slots, transpose patches).  The lane-level replays must keep agreeing
    with the dense computation (they assert it themselves)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("mfma_chain_emu.py", "xattn_full_emu.py", "ff_fused_emu.py"):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "experiments", "next", name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-400:], r.stderr[-400:])
        assert "e-1" in r.stdout, (name, r.stdout)      # 1e-15-class agreement printed by each script


# keys of the parity record the documents quote numbers from (README.md); tools/commit_parity.py
# refuses a record that lacks one of them
PARITY_KEYS_CITED = ["unet_forward_full_64x48_n16_vs_oracle", "config2_chain_B2_20_pndm_vs_oracle", "tryon_512x384_50_pndm_B8_vs_oracle",
                     "tryon_1024x768_100_ddim_B1_vs_oracle"]


def test_committed_parity_record_is_one_run_and_holds_every_cited_key():
    """profiles/r06_parity.json is ONE full `pytest -m gpu` run on one binary (tests/util.py record_parity stamps the library digest and the
    session id; tests/conftest.py starts every GPU session from an empty record) and holds every key the documents cite -- explicitly listed
    above, plus every `..._vs_oracle` key a document names in back-ticks (the round-4 file was a 3-key fragment that lacked the
    key BASELINE.md quoted)."""
    import json
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "r06_parity.json")
    if not os.path.exists(path):
        pytest.skip("no round-6 parity record committed yet")
    blob = json.load(open(path))
    assert re.fullmatch(r"[0-9a-f]{64}", blob.get("_library_digest", "")), "the record names the library it was taken on"
    assert blob.get("_session"), "the record names its pytest session"
    cited = set(PARITY_KEYS_CITED)
    for doc in ("DESIGN.md", "BASELINE.md", "README.md", os.path.join("profiles", "README.md")):
        cited.update(k for k in re.findall(r"`([a-z0-9_]+_vs_oracle)`", open(os.path.join(root, doc)).read()) if not k.startswith("test_"))   # (test names end the same way)
    missing = sorted(k for k in cited if k not in blob)
    assert not missing, missing
    assert len([k for k in blob if not k.startswith("_")]) >= 12, "a full GPU run records every measured tolerance, not a fragment"



def test_halo_weight_slice_major_map_covers_every_tile_once():
    """Host-side replay of igemm_halo_kernel.h's tile_map 3 decode (round 6): block b -> XCD b % 8, unit = (channel tile, K slice, group of G pixel
    tiles), the G workgroups of a unit consecutive on ONE XCD.  Every (qt, pt, z) must be produced exactly once, the surplus blocks must return,
    and all workgroups of a unit must share b % 8 -- for the launch populations the library uses it on and a few awkward ones."""
    def decode(b, nq, np_, S, G):
        npg = (np_ + G - 1) // G
        xcd, loc = b & 7, b >> 3
        ui, pi = loc // G, loc % G
        u = ui * 8 + xcd
        if u >= nq * S * npg:
            return None
        pg, qz = u % npg, u // npg
        pt, qt, z = pg * G + pi, qz // S, qz % S
        return None if pt >= np_ else (qt, pt, z, u, xcd)

    for nq, np_, S in ((10, 24, 2), (10, 6, 4), (10, 16, 2), (5, 24, 1), (3, 13, 3), (7, 32, 2), (1, 2, 1)):
        G = np_ if np_ <= 12 else (np_ + 1) // 2                     # the launcher's choice
        units = nq * S * ((np_ + G - 1) // G)
        blocks = 8 * ((units + 7) // 8) * G
        seen, unit_xcd = {}, {}
        for b in range(blocks):
            d = decode(b, nq, np_, S, G)
            if d is None:
                continue
            qt, pt, z, u, xcd = d
            assert (qt, pt, z) not in seen, (nq, np_, S, qt, pt, z)
            seen[(qt, pt, z)] = b
            assert unit_xcd.setdefault(u, xcd) == xcd                # one XCD per unit
        assert len(seen) == nq * np_ * S, (nq, np_, S, len(seen))
        for u in unit_xcd:                                           # the workgroups of a unit are G CONSECUTIVE blocks of their XCD's sequence
            bs = sorted(b for (qt, pt, z), b in seen.items() if (qt * S + z) * ((np_ + G - 1) // G) + pt // G == u)
            locs = [b >> 3 for b in bs]
            assert locs == list(range(locs[0], locs[0] + len(locs))), (nq, np_, S, u)


def test_halo_folded_upsample_tables_emulation():
    """Host-side replay of the folded-upsample halo form's addressing (igemm_halo_kernel.h UPS, round 6): the staged tile is the run of LOW-resolution
    rows from source row (y0 - 1) >> 1 of the tile's first output row on; tap (dy, dx) of output pixel (y, x) reads staged row
    (((y + dy - 1) >> 1) - r0) * Ws + ((x + dx - 1) >> 1), masked where the tap leaves the 2H x 2W image.  Replayed in numpy against
    conv2d(interpolate(x, 2, nearest)) for tiles that start in the middle of an image row, first / last tiles of a sample and several tile sizes."""
    import numpy as np
    rng = np.random.default_rng(3)
    F_ = torch.nn.functional
    for (Hs, Ws, BP, rows_cap) in ((12, 24, 192, 290), (8, 12, 192, 242), (16, 12, 128, 226), (4, 8, 128, 226), (6, 4, 32, 64)):
        Ho, Wo = 2 * Hs, 2 * Ws
        assert (Ho * Wo) % BP == 0
        x = rng.standard_normal((Hs * Ws,)).astype(np.float64)      # one channel is enough: the addressing is channel-independent
        w = rng.standard_normal((3, 3)).astype(np.float64)
        ref = F_.conv2d(F_.interpolate(torch.from_numpy(x).view(1, 1, Hs, Ws), scale_factor=2.0, mode="nearest"), torch.from_numpy(w).view(1, 1, 3, 3), padding=1).view(-1).numpy()
        got = np.zeros(Ho * Wo)
        for q0 in range(0, Ho * Wo, BP):
            y0, y1 = q0 // Wo, (q0 + BP - 1) // Wo
            r0 = (y0 - 1) >> 1
            l0 = r0 * Ws
            u_rows = (((y1 + 1) >> 1) - r0 + 1) * Ws
            assert u_rows <= rows_cap                                # fits the halo buffer of the form that takes this shape
            tile = np.zeros(u_rows)
            for r in range(u_rows):                                  # DMA side: source pixel l0 + r, zero-filled outside the sample
                lin = l0 + r
                tile[r] = x[lin] if 0 <= lin < Hs * Ws else 0.0
            for pl in range(BP):
                q = q0 + pl
                oy, ox = q // Wo, q % Wo
                acc = 0.0
                for dy in range(3):
                    for dx in range(3):
                        if not (0 <= oy + dy - 1 < Ho and 0 <= ox + dx - 1 < Wo):
                            continue                                 # the validity bit: the lane reads the zero row
                        row = (((oy + dy - 1) >> 1) - r0) * Ws + ((ox + dx - 1) >> 1)
                        assert 0 <= row < u_rows
                        acc += tile[row] * w[dy, dx]
                got[q] = acc
        assert np.allclose(got, ref, atol=1e-12), (Hs, Ws, BP)


def test_gn_reduce_rows_fold_emulation():
    """Host-side replay of norm.hip gn_reduce_rows_kernel (round 6): block (b, n) folds partial rows [b rps / 16, (b + 1) rps / 16) -- row lanes of
    one float4 (two channels) each, four rows in flight, the lanes combined in lane order -- into 16 rows per sample whose sum is the sum of all rows;
    including the C = 320 case (160 float4 pieces per row: ONE row lane, the threads beyond piece 159 must write nothing -- the race fixed this round)."""
    import numpy as np
    rng = np.random.default_rng(5)
    for C, rps in ((128, 6144), (320, 123), (512, 768), (256, 97), (1280, 200)):
        part = rng.standard_normal((rps, C, 2))
        q = C // 2
        lanes = 256 // q if q < 256 else 1
        out = np.full((16, C, 2), np.nan)
        for b in range(16):
            r_lo, r_hi = b * rps // 16, (b + 1) * rps // 16
            for q0 in range(0, q, 256):
                acc = np.zeros((256, 4))
                live = np.zeros(256, bool)
                for tid in range(256):
                    qi = q0 + (tid % q if q < 256 else tid)
                    rl = tid // q if q < 256 else 0
                    if rl < lanes and qi < q:
                        live[tid] = True
                        for r in range(r_lo + rl, r_hi, lanes):
                            acc[tid] += part[r].reshape(-1)[4 * qi:4 * qi + 4]
                if lanes > 1:
                    for tid in range(q):
                        t = sum(acc[l * q + tid] for l in range(lanes))
                        out[b].reshape(-1)[4 * tid:4 * tid + 4] = t
                else:
                    for tid in range(256):
                        qi = q0 + (tid % q if q < 256 else tid)
                        if live[tid]:                                 # (the fixed kernel: `rl < lanes && qi < q`)
                            out[b].reshape(-1)[4 * qi:4 * qi + 4] = acc[tid]
        assert not np.isnan(out).any()
        assert np.allclose(out.sum(0), part.sum(0), rtol=1e-10, atol=1e-9), (C, rps)


def test_one_pass_group_norm_chunk_math_emulation():
    """Host-side replay of norm.hip gn_norm_kernel's index arithmetic (round 5): a block owns a 64-channel chunk, sums the partial rows of every
    group that overlaps the chunk (groups straddle chunk boundaries and the boundary of the two concat sources; the last chunk may be ragged),
    and applies scale / shift to its own channels only.  Replayed with the kernel's own formulas (row lanes, statistic-channel range
    [g_lo gs, (g_hi + 1) gs)) in numpy and compared with GroupNorm over the virtual concat -- also in the 'direct' form (no partial rows: the
    statistics come from the data), which the 48-pixel samples of the 8x6 level take."""
    import numpy as np
    rng = np.random.default_rng(0)

    def replay(x0, x1, groups, gamma, beta, eps, rows_px):
        N, HW, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[2]
        Ct, gs = C0 + C1, (C0 + C1) // groups
        parts = []
        for x in (x0, x1):
            if x is None or rows_px == 0:
                parts.append(None)
                continue
            rps = HW // rows_px
            blk = x.reshape(N, rps, rows_px, x.shape[2])
            parts.append(np.stack([blk.sum(2), (blk ** 2).sum(2)], -1))        # [N][rps][C][2]
        out = np.zeros((N, HW, Ct))
        for n in range(N):
            for z in range((Ct + 63) // 64):
                c0 = z * 64
                nch = min(64, Ct - c0)
                g_lo, g_hi = c0 // gs, (c0 + nch - 1) // gs
                ng, cb = g_hi - g_lo + 1, g_lo * gs
                ncs = ng * gs
                assert ncs <= 256 and ng <= 66 and cb + ncs <= Ct
                RL = 256 // ncs
                rsum, rsq = np.zeros((RL, ncs)), np.zeros((RL, ncs))
                for tid in range(256):
                    cl, rl = tid % ncs, tid // ncs
                    if rl >= RL:
                        continue
                    c = cb + cl
                    src, part, clc = (x0, parts[0], c) if c < C0 else (x1, parts[1], c - C0)
                    if part is not None:
                        for r in range(rl, part.shape[1], RL):
                            rsum[rl, cl] += part[n, r, clc, 0]; rsq[rl, cl] += part[n, r, clc, 1]
                    else:
                        for r in range(rl, HW, RL):
                            rsum[rl, cl] += src[n, r, clc]; rsq[rl, cl] += src[n, r, clc] ** 2
                csum, csq = rsum.sum(0), rsq.sum(0)
                mean = np.array([csum[g * gs:(g + 1) * gs].sum() for g in range(ng)]) / (gs * HW)
                var = np.maximum(np.array([csq[g * gs:(g + 1) * gs].sum() for g in range(ng)]) / (gs * HW) - mean ** 2, 0)
                rstd = 1 / np.sqrt(var + eps)
                for c in range(c0, c0 + nch):
                    g = c // gs - g_lo
                    sc = gamma[c] * rstd[g]
                    src = x0[n, :, c] if c < C0 else x1[n, :, c - C0]
                    out[n, :, c] = src * sc + (beta[c] - mean[g] * sc)
        return out

    for (C0, C1, groups, HW, rows_px) in ((320, 0, 32, 96, 32), (640, 320, 32, 64, 32), (160, 0, 32, 48, 0), (96, 32, 32, 48, 0), (1920, 640, 32, 48, 0)):
        x0 = rng.normal(size=(2, HW, C0)) * 2 + 0.5
        x1 = rng.normal(size=(2, HW, C1)) if C1 else None
        gamma, beta = 1 + 0.1 * rng.normal(size=C0 + C1), 0.1 * rng.normal(size=C0 + C1)
        got = replay(x0, x1, groups, gamma, beta, 1e-5, rows_px)
        xc = np.concatenate([x0, x1], 2) if C1 else x0
        xg = xc.reshape(2, HW, groups, -1)
        ref = ((xg - xg.mean((1, 3), keepdims=True)) / np.sqrt(xg.var((1, 3), keepdims=True) + 1e-5)).reshape(2, HW, -1) * gamma + beta
        assert np.abs(got - ref).max() < 1e-9, (C0, C1, HW)


def test_halo_2d_block_addressing_emulation():
    """Host-side replay of the 2-D blocked halo tile's addressing (igemm_halo.hip G2D, round 5): block pt -> (sample, block row, block column);
    staged row i of the (TH + 2) x 34 block -> image pixel (or the zero frame); consumer row of output pixel (r, col) = (r + 1) 34 + col + 1; a tap
    is the linear shift (dy - 1) 34 + (dx - 1).  For every output pixel and tap the staged value read must be the zero-padded 3x3 neighbour."""
    import numpy as np
    rng = np.random.default_rng(1)
    for (N, H, W, TH) in ((2, 16, 64, 8), (1, 8, 96, 4), (3, 4, 32, 4)):
        img = rng.integers(1, 1000, size=(N, H, W)).astype(np.int64)
        txn, tps = W // 32, (H // TH) * (W // 32)
        HC = 34
        for pt in range(N * tps):
            n, t = pt // tps, pt % tps
            ty, tx = t // txn, t % txn
            y0, x0 = ty * TH, tx * 32
            p0 = (n * H + y0) * W + x0
            staged = np.zeros(((TH + 2) * HC + 64,), dtype=np.int64)           # rows beyond the block: zero-filled passes
            for i in range((TH + 2) * HC):
                rr, cc = i // HC, i % HC
                y, x = y0 - 1 + rr, x0 - 1 + cc
                if 0 <= y < H and 0 <= x < W:
                    staged[i] = img[n, y, x]
            for r in range(TH):                                                 # sub-tile r = image row y0 + r, epilogue pixel index p0 + r W + col
                for col in range(32):
                    rb = (r + 1) * HC + col + 1
                    assert p0 + r * W + col == (n * H + y0 + r) * W + x0 + col
                    for tap in range(9):
                        dy, dx = tap // 3, tap % 3
                        got = staged[rb + (dy - 1) * HC + (dx - 1)]
                        y, x = y0 + r + dy - 1, x0 + col + dx - 1
                        assert got == (img[n, y, x] if 0 <= y < H and 0 <= x < W else 0)
