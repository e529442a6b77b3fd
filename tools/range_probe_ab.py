"""Cost of the range probe on the released UNet (n = 16, 64 x 48 latents), arms interleaved on the same GPU:

  * probe OFF against another build of the library (--parent-lib: the parent commit's libladi_native.so): ladi_unet_time_forward of
    both, one process per arm and round, alternating; the difference has to sit inside the spread of the repeated parent arm;
  * probe ON: the same forward with a RangeProbe attached;
  * the probe kernel alone on the forward's largest tensor ([16 * 64 * 48][320] fp16, 31.5 MB): device-event time over many launches, on
    one buffer (resident in the 256 MB Infinity Cache after the first pass) and rotating over 20 buffers (629 MB: every pass from HBM).

    python tools/range_probe_ab.py --parent-lib PATH [--out profiles/range_probe_off_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def open_lib(path):
    """a second copy of the library next to the package's own: typed like _lib.load() for the symbols it has"""
    from ladi_vton_amd import _lib
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def child(a):
    """one arm in a process of its own: UNet on the library at a.child, warm-up, a.reps timed figures -> one JSON line"""
    import json
    from ladi_vton_amd import _lib
    _lib._lib = open_lib(a.child)                      # before anything binds the package's own copy
    import ladi_vton_amd as L
    from ladi_vton_amd import configs as C
    unet = L.NativeUNet(C.UNET_FULL, C.synth_state_dict(C.unet_shapes(C.UNET_FULL), "unet."))
    probe = L.RangeProbe().attach(unet) if a.probe else None
    n, h, w = 16, 64, 48
    unet.set_context(torch.randn((n, 77, C.UNET_FULL["cross_attention_dim"]), generator=torch.Generator().manual_seed(1)).half().cuda())
    unet.time_forward(n, h, w, 2); unet.time_forward(n, h, w, 2)       # warm-up: tile measurement of every shape, code objects
    ms = [unet.time_forward(n, h, w, a.iters) for _ in range(a.reps)]
    if probe:
        assert probe.first_nonfinite() is None and len(probe.names()) == len(L.probe.unet_point_names(C.UNET_FULL))
        probe.detach()
    print("AB_RESULT " + json.dumps(ms), flush=True)


def run_child(lib, probe, a):
    import json
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--probe", str(probe), "--iters", str(a.iters), "--reps", str(a.reps)],
                       capture_output=True, text=True, timeout=300)
    for ln in r.stdout.splitlines():
        if ln.startswith("AB_RESULT "):
            return json.loads(ln[len("AB_RESULT "):])
    raise RuntimeError("arm failed (rc=%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_probe_off_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child")
    ap.add_argument("--probe", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    from ladi_vton_amd import _lib
    n, h, w = 16, 64, 48
    arms = {"parent": [], "new_off": [], "new_on": []}
    spec = {"parent": (os.path.abspath(a.parent_lib), 0), "new_off": (_lib.LIB_PATH, 0), "new_on": (_lib.LIB_PATH, 1)}
    rows_ = []
    for r in range(a.rounds):                          # one process per arm and round, one at a time, arms alternating
        for arm in (["parent", "new_off", "new_on"] if r % 2 == 0 else ["new_on", "new_off", "parent"]):
            ms = run_child(spec[arm][0], spec[arm][1], a)
            arms[arm] += ms
            rows_.append("round %d  %-8s %s" % (r, arm, "  ".join("%.4f" % x for x in ms)))
            print(rows_[-1], flush=True)
    import ladi_vton_amd as L
    from ladi_vton_amd import configs as C
    new_lib = _lib.load()
    lines = ["range probe cost, UNet full size, n = %d, %d x %d latents, %s" % (n, h, w, torch.cuda.get_device_name(0)),
             "ladi_unet_time_forward, ms per forward (%d forwards per figure, %d figures per process after two warm-up calls);" % (a.iters, a.reps),
             "arms: parent = the parent commit's library, new_off = this library without a probe, new_on = with a RangeProbe attached;",
             "one process per arm and round, run one after the other on the same GPU, order alternating", ""] + rows_
    med = {k: statistics.median(v) for k, v in arms.items()}
    lines += ["", "median  parent %.4f  new(probe off) %.4f  new(probe on) %.4f" % (med["parent"], med["new_off"], med["new_on"]),
              "parent arm spread (min .. max) %.4f .. %.4f = %.3f %% of its median" % (min(arms["parent"]), max(arms["parent"]),
                                                                                    100 * (max(arms["parent"]) - min(arms["parent"])) / med["parent"]),
              "probe off - parent: %+.4f ms (%+.3f %%)" % (med["new_off"] - med["parent"], 100 * (med["new_off"] - med["parent"]) / med["parent"]),
              "probe on  - probe off: %+.4f ms (%+.3f %%), %d probe launches per forward" % (med["new_on"] - med["new_off"],
                                                                                         100 * (med["new_on"] - med["new_off"]) / med["new_off"],
                                                                                         len(L.probe.unet_point_names(C.UNET_FULL)))]
    inside = min(arms["parent"]) <= med["new_off"] <= max(arms["parent"])
    lines.append("probe-off median inside the parent arm's spread: %s" % ("yes" if inside else "NO"))
    # ---- the kernel alone
    rows, Cc = n * h * w, 320
    nbytes = rows * Cc * 2
    bufs = [torch.randn((rows, Cc), device="cuda", dtype=torch.float16) for _ in range(20)]
    am = torch.zeros(1, dtype=torch.float32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(k, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(20):
            new_lib.ladi_op_absmax(_lib.ptr(bufs[i % k]), rows, Cc, Cc, _lib.ptr(am), _lib.ptr(nf), _lib.stream_ptr())
        e0.record()
        for i in range(reps):
            new_lib.ladi_op_absmax(_lib.ptr(bufs[i % k]), rows, Cc, Cc, _lib.ptr(am), _lib.ptr(nf), _lib.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    lines += ["", "absmax_probe_kernel alone, [%d][%d] fp16 = %.1f MB per launch, 2000 launches per figure (device events, launch gaps included)" % (rows, Cc, nbytes / 1e6)]
    for k, what in ((1, "one buffer (Infinity-Cache resident)"), (20, "20 buffers in turn (629 MB, from HBM)")):
        t = [run(k, 2000) for _ in range(3)]
        ms = statistics.median(t)
        lines.append("%-40s %.2f us per launch, %.0f GB/s = %.1f %% of the 8 TB/s nominal HBM rate (runs: %s)" % (
            what, 1e3 * ms, nbytes / ms / 1e6, 100 * nbytes / ms / 1e6 / 8000.0, ", ".join("%.2f" % (1e3 * x) for x in t)))
    assert float(am) == max(float(b.abs().max()) for b in bufs) and int(nf) == 0
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
