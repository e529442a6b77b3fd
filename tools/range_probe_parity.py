"""Range probe against the fp32 oracle: one UNet forward of the tiny and of the released configuration under a RangeProbe, every probe
point's magnitude compared with oracle max |x| (tests/range_probe_ref.py).  Writes the per-point and worst relative differences as JSON
(committed as profiles/range_probe_parity.json; tests/test_gpu_range_probe.py asserts 4x the tiny figure).

    python tools/range_probe_parity.py [--out profiles/range_probe_parity.json] [--skip-full]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(cfg, n, h, w, L_, seed):
    import ladi_vton_amd as L
    from ladi_vton_amd import configs as C
    from tests import range_probe_ref as R
    sd = C.synth_state_dict(C.unet_shapes(cfg), "unet.")
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cfg["in_channels"], h, w), generator=g).half().float()
    ehs = torch.randn((n, L_, cfg["cross_attention_dim"]), generator=g).half().float()
    ref, _ = R.unet_point_absmax(sd, cfg, x, 481, ehs)
    unet = L.NativeUNet(cfg, sd)
    probe = L.RangeProbe().attach(unet)
    unet(x.cuda(), 481, encoder_hidden_states=ehs.cuda())
    rep = probe.report()
    probe.detach()
    assert [r[0] for r in rep] == list(ref)
    rel = {name: abs(a - ref[name]) / ref[name] for name, a, _, _ in rep}
    worst = max(rel, key=rel.get)
    return dict(shape=[n, cfg["in_channels"], h, w], context_len=L_, worst_rel=rel[worst], worst_point=worst,
                nonfinite=int(sum(r[3] for r in rep)),
                points={name: dict(native=a, oracle=ref[name], rel=rel[name]) for name, a, _, _ in rep})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_probe_parity.json"))
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()
    from ladi_vton_amd import configs as C
    res = dict(what="range probe absmax vs fp32 oracle max|x|, relative difference per UNet probe point, one forward",
               device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count)
    res["tiny"] = measure(C.UNET_TINY, 2, 16, 16, 8, 5)        # the input of tests/test_gpu_range_probe.py
    print("tiny: worst %.3e at %s" % (res["tiny"]["worst_rel"], res["tiny"]["worst_point"]), flush=True)
    if not a.skip_full:
        res["full"] = measure(C.UNET_FULL, 1, 64, 48, 77, 7)
        print("full: worst %.3e at %s" % (res["full"]["worst_rel"], res["full"]["worst_point"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
