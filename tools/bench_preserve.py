"""Keeping the unmasked region (`preserve_unmasked=`) against the plain run, on one GPU.

    plain     512x384, B = 8, 50 PNDM steps (BASELINE configs[1]): the fused run as bench.py runs it
    latents   the same run with the latent blend (one more VAE encode, the blend inside the step kernel)
    pixels    the same run with the composite decode epilogue (--feather: the feathered mask, two more launches)
    both      both

Full-size random-init checkpoint and bench.py's synthetic rows.  Every arm has its own native handle (its graphs stay captured), the arms are
interleaved (plain, latents, pixels, both, plain, ..) for --iters repetitions after --warmup untimed rounds, in one process.  Per arm: the
library's three stage times (preprocess + encodes + EMASC, denoising loop, decode) and the whole call's HIP-event time, medians with every
run listed.  No threshold is applied: the numbers are a record.  Prints one JSON line.

--plain-only times the plain arm alone and passes no new argument, so with --root it runs against another checkout of this repository (the
parent commit with its own library): run the two alternately on one box for the A/B of the plain path.
--table renders the JSON lines of earlier runs (files) as the markdown BASELINE.md holds; --write-baseline puts it between the markers there.

    python tools/bench_preserve.py [--batch 8] [--iters 5] [--warmup 2] [--feather 0] [--plain-only] [--root DIR] [--label parent]
    python tools/bench_preserve.py --table run.json [--ab new1.json parent1.json ..] [--write-baseline]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, STEPS = 512, 384, 50
BEGIN, END = "<!-- bench_preserve:begin -->", "<!-- bench_preserve:end -->"


def measure(a):
    root = os.path.abspath(a.root) if a.root else HERE
    sys.path.insert(0, root)
    import torch

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

    def pipe():      # one native handle per arm: no arm re-captures its graphs when another has run
        return L.StableDiffusionTryOnePipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, scheduler=L.PNDMScheduler(), emasc=emasc,
                                               emasc_int_layers=[1, 2, 3, 4, 5])
    arms = [dict(name="plain", kw={}, pipe=pipe())]
    if not a.plain_only:
        for name, bits in (("latents", 1), ("pixels", 2), ("both", 3)):
            arms.append(dict(name=name, kw=dict(preserve=(bits, float(a.feather) if bits & 2 else 0.0)), pipe=pipe()))
    for arm in arms:
        arm.update(stage_ms=[], seconds=[])

    def run(arm, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        arm["pipe"]._run_fused(rows["image"], rows["mask_image"], rows["pose_map"], rows["warped_cloth"], rows["prompt_embeds"],
                               rows["negative_prompt_embeds"], rows["noise_cloth"], rows["noise_latents"], rows["noise_masked"], H, W, STEPS,
                               7.5, 1.0, False, True, return_device=True, out_uint8=True, **arm["kw"])
        e1.record()
        torch.cuda.synchronize()
        if arm["pipe"].check_overflow():
            raise RuntimeError("a VAE decode left the fp16 range: the run is not a measurement")
        if timed:
            ms = (ctypes.c_float * 3)()
            if lib.ladi_tryon_stage_ms(arm["pipe"]._tryon, ms) != 0:
                raise RuntimeError("no stage times")
            arm["stage_ms"].append(list(ms))
            arm["seconds"].append(e0.elapsed_time(e1) / 1e3)
    for r in range(a.warmup + a.iters):      # interleaved: every round runs every arm once
        for arm in arms:
            run(arm, r >= a.warmup)
    out = []
    for arm in arms:
        st = [statistics.median(s[i] for s in arm["stage_ms"]) for i in range(3)]
        sec = statistics.median(arm["seconds"])
        out.append(dict(arm=arm["name"], encode_ms=st[0], loop_ms=st[1], decode_ms=st[2], seconds=sec, seconds_runs=arm["seconds"],
                        stage_ms_runs=arm["stage_ms"], images_per_s=B / sec))
    print(json.dumps({"metric": "preserve_seconds_per_batch", "batch": B, "size": a.size, "device": torch.cuda.get_device_name(0),
                      "what": "%dx%d, %d PNDM steps, CFG 7.5, uint8 output on the device" % (H, W, STEPS), "iters": a.iters, "warmup": a.warmup,
                      "feather": a.feather, "label": a.label, "arms": out}))


def _last_json(path):
    with open(path) as fh:
        lines = [ln for ln in fh if ln.lstrip().startswith("{")]
    return json.loads(lines[-1])


def table(a):
    res = _last_json(a.table)
    plain = res["arms"][0]
    md = ["%s, B = %d, %s; %d interleaved rounds after %d warm-up rounds, medians (ms)." % (res["device"], res["batch"], res["what"], res["iters"],
                                                                                         res["warmup"]), "",
          "| arm | encodes + EMASC | loop | decode | whole call | vs plain |", "|---|---|---|---|---|---|"]
    for e in res["arms"]:
        md.append("| %s%s | %.2f | %.2f | %.2f | %.2f | %+.2f ms (%+.2f %%) |"
                  % (e["arm"], " (feather %g)" % res["feather"] if res["feather"] and e["arm"] in ("pixels", "both") else "", e["encode_ms"],
                     e["loop_ms"], e["decode_ms"], 1e3 * e["seconds"], 1e3 * (e["seconds"] - plain["seconds"]),
                     100 * (e["seconds"] / plain["seconds"] - 1)))
    if a.ab:
        md += ["", "Plain run, this library against the parent commit's, processes run alternately on the same box (median of each process, ms):", "",
               "| process | library | loop | whole call |", "|---|---|---|---|"]
        for i, path in enumerate(a.ab):
            r = _last_json(path)
            md.append("| %d | %s | %.2f | %.2f |" % (i + 1, r.get("label") or "this", r["arms"][0]["loop_ms"],
                                                    1e3 * r["arms"][0]["seconds"]))
    text = "\n".join(md) + "\n"
    print(text)
    if a.write_baseline:
        path = os.path.join(HERE, "BASELINE.md")
        with open(path) as fh:
            doc = fh.read()
        if BEGIN not in doc or END not in doc:
            raise SystemExit("BASELINE.md has no %s / %s markers" % (BEGIN, END))
        head, rest = doc.split(BEGIN, 1)
        tail = rest.split(END, 1)[1]
        with open(path, "w") as fh:
            fh.write(head + BEGIN + "\n" + text + END + tail)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--feather", type=float, default=0.0)
    p.add_argument("--size", default="full", choices=["full", "tiny"])
    p.add_argument("--plain-only", action="store_true")
    p.add_argument("--root", default=None)
    p.add_argument("--label", default="this")
    p.add_argument("--table", default=None)
    p.add_argument("--ab", nargs="*", default=[])
    p.add_argument("--write-baseline", action="store_true")
    a = p.parse_args()
    table(a) if a.table else measure(a)


if __name__ == "__main__":
    main()
