"""What the denoiser's spatial variance estimate costs, and that plain frames and the plain denoise call cost
what they did: in ONE process on one GPU.

    python tools/spatial_variance_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

(a) As tools/denoise_timing.py: on bench.py's C2 and C3 scenes every round times pbr_hip_render of a library
built from the parent commit (--parent; skipped without it) and of this build, alternating; then the same for a
plain pbr_hip_denoise call (no estimate; 5 levels, all three outputs, 1920x1080 and 3840x2160, the synthetic
8-sample frame of that tool), whose rgb must have the same bits from both libraries.  A variant's time is the
host clock around `steps` calls queued back to back on one stream, ending in a synchronise, divided by `steps`.
This build may not be slower than the parent by more than the larger of the two spreads ((max - min) / median
over the rounds; the parent is the yardstick); the tool says PASS or FAIL.

(b) k_dn_spatial's event time (pbr_hip_set_profiling) at both sizes for each radius, median over the rounds, on
a frame whose pixels all hold one sample (every pixel takes the estimate) and on one whose pixels all hold 8
(none does: every tile copies its pixels and stages nothing), beside the level-0 time of the same run and the
achieved bytes per second over the kernel's compulsory traffic — 68 B per pixel: colour/variance, moments/count
and guides read, the slope read, colour/variance written — beside the 6.29 TB/s a float4 copy measures on this
GPU.  (A tile that only copies moves 36 B per pixel — the count, the colour read and written — so on the frame
where no pixel estimates the 68-byte figure overstates the rate.)  A first measurement: no speed is required of
the estimate."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pysicalbasedraytracer_amd import capi  # noqa: E402
from denoise_timing import HBM_COPY_TBS, SIZES, plain_frames, renderer, stat, synthetic  # noqa: E402

SPATIAL_BYTES = 68    # per pixel: read x/V, u/n, N/z (16 each) and g (4), write x/V (16)
LEVEL_BYTES = 48
MIN_COUNT = 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libpbr_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--configs", nargs="*", default=["C2", "C3"], choices=["C2", "C3", "C5"])
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--md", help="write the result lines as a markdown document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spatial_variance_timing: no GPU (times are measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    this = capi.load_library()
    parent = capi.load_library(os.path.abspath(a.parent)) if a.parent else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"this build: {this.pbr_hip_build_info().decode()}")
    if parent:
        say(f"parent:     {parent.pbr_hip_build_info().decode()}")
    out = {"rounds": a.rounds, "steps": a.steps, "levels": a.levels, "configs": {}, "denoise": {}, "spatial": {}}
    # ---- (a) plain frames against the parent's
    ok = plain_frames(a, this, parent, dev, st, say, out)
    # ---- (a) the plain denoise call against the parent's
    frames = {}
    for (W, H) in SIZES:
        n = W * H
        frames[W, H] = synthetic(dev, W, H, 8) + (torch.empty((n, 3), dtype=torch.float32, device=dev),
                                                  torch.empty((n, 4), dtype=torch.uint8, device=dev),
                                                  torch.empty((n,), dtype=torch.float32, device=dev))
    torch.cuda.synchronize(dev)

    def call(r, W, H, samples=8, acc=None, spatial=None):
        acc0, aov, rgb, rgba, var = frames[W, H]
        r.denoise(W, H, samples, (acc if acc is not None else acc0).data_ptr(), aov.data_ptr(), rgb_ptr=rgb.data_ptr(),
                  rgba_ptr=rgba.data_ptr(), var_ptr=var.data_ptr(), iterations=a.levels, stream=st, spatial=spatial)

    names = (["denoise/parent"] if parent else []) + ["denoise"]
    for (W, H) in SIZES:
        times = {n: [] for n in names}
        ref = None
        for rnd in range(a.rounds):
            for name in names:
                r = renderer(parent if name == "denoise/parent" else this)   # one context at a time
                frames[W, H][2].fill_(float("nan"))
                torch.cuda.synchronize(dev)
                call(r, W, H)   # warm-up: the planes are allocated here
                r.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(r, W, H)
                r.sync()
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[name].append(ms)
                bits = frames[W, H][2].cpu().numpy().view(np.uint32)   # this build computes what the parent computed
                if ref is None:
                    ref = bits.copy()
                same = np.array_equal(bits, ref)
                print(f"denoise {W}x{H} round {rnd} {name:15s} {ms:10.3f} ms{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"denoise {W}x{H} {name}: the filtered image differs between the builds or the rounds")
        res = {name: stat(times[name]) for name in names}
        for name in names:
            v = res[name]
            say(f"RESULT denoise {W}x{H}, {a.levels} levels, {name:15s} median {v['median_ms']:8.3f} ms (min {v['min_ms']:.3f}, "
                f"max {v['max_ms']:.3f}, spread {100 * v['spread']:.2f}%)")
        if parent:
            p, t = res["denoise/parent"], res["denoise"]
            slower = t["median_ms"] / p["median_ms"] - 1
            bound = max(p["spread"], t["spread"])
            verdict = "PASS" if slower <= bound else "FAIL"
            ok = ok and slower <= bound
            say(f"RESULT denoise {W}x{H} (a) plain call vs parent: {100 * slower:+.2f}% (bound: the larger spread, "
                f"{100 * bound:.2f}%) {verdict}; the bits are equal")
            res["plain_vs_parent"] = {"slower": slower, "bound": bound, "pass": slower <= bound}
        out["denoise"][f"{W}x{H}"] = res
    # ---- (b) the estimate
    r = renderer(this)
    r.set_profiling(True)
    for (W, H) in SIZES:
        one = synthetic(dev, W, H, 1)[0]
        torch.cuda.synchronize(dev)
        for radius in (1, 2, 3):
            for label, samples, acc in (("every pixel estimates (1 sample)", 1, one), ("no pixel estimates (8 samples)", 8, None)):
                call(r, W, H, samples, acc, (MIN_COUNT, radius))   # warm-up (the fifth plane)
                r.sync()
                r.get_profile()
                sp, l0, prep = [], [], []
                for rnd in range(a.rounds):
                    call(r, W, H, samples, acc, (MIN_COUNT, radius))
                    r.sync()
                    prof = r.get_profile()
                    sp.append(prof["k_dn_spatial"]["ms"])
                    l0.append(prof["k_dn_atrous_l0"]["ms"])
                    prep.append(prof["k_dn_prepare"]["ms"])
                n = W * H
                ms, ms0 = statistics.median(sp), statistics.median(l0)
                tbs = SPATIAL_BYTES * n / (ms * 1e-3) / 1e12
                tbs0 = LEVEL_BYTES * n / (ms0 * 1e-3) / 1e12
                say(f"RESULT spatial {W}x{H} r={radius} {label}: k_dn_spatial {ms:.3f} ms (min {min(sp):.3f}, max {max(sp):.3f}), "
                    f"{SPATIAL_BYTES} B/pixel compulsory = {tbs:.2f} TB/s, {100 * tbs / HBM_COPY_TBS:.0f}% of the {HBM_COPY_TBS} TB/s "
                    f"copy rate; level 0 of the same runs {ms0:.3f} ms ({tbs0:.2f} TB/s over {LEVEL_BYTES} B/pixel); prepare with "
                    f"the moments plane {statistics.median(prep):.3f} ms")
                out["spatial"][f"{W}x{H} r={radius} {label}"] = {"ms": sp, "median_ms": ms, "level0_ms": l0, "prepare_ms": prep,
                                                                "tb_per_s": tbs}
    r.set_profiling(False)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# The denoiser's spatial variance estimate: timing\n\n`tools/spatial_variance_timing.py` on one MI355X; every "
                    "line below is the tool's output.  These are the first measurements of this kernel.\n\n```\n" +
                    "\n".join(lines) + "\n```\n")
    if not ok:
        sys.exit("spatial_variance_timing: a plain frame or the plain denoise call is slower than the parent's by more than "
                 "the measured spread")


if __name__ == "__main__":
    main()
