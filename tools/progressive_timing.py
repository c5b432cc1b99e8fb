"""What progressive rendering costs: sample passes against whole frames, in ONE process on one GPU.

    python tools/progressive_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 7] [--steps 5] [--json out.json]

On bench.py's C2 scene (1920x1080, 64 spp) every round times, one after the other,
  plain/parent   pbr_hip_render of a library built from the parent commit (--parent; skipped without it)
  plain          pbr_hip_render of this build
  8x8            8 passes of 8 samples in one pbr_hip_render_passes call
  64x1           64 passes of 1 sample in one call
  8x8/calls      the same 8 passes as eight separate asynchronous calls
and on C3 (256 spp, Sobol) plain/parent, plain and 4 passes of 64 in one call.  A variant's time is
the host clock around `steps` frames queued back to back on one stream, ending in a synchronise,
divided by `steps` (bench.py's timed window).  The rounds alternate the variants, so drift of the
machine reaches all of them alike; per variant the tool prints median, min and max over the rounds,
and the spread (max - min) / median of the parent's plain frame, the yardstick for every difference
below.  Every variant's last image must equal the plain frame of this build bit for bit."""
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
from pysicalbasedraytracer_amd import HipRenderer, capi, scenes  # noqa: E402


def renderer(lib, scene):
    capi._lib = lib   # HipRenderer() binds the library loaded last
    r = HipRenderer(0)
    r.upload(scene)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libpbr_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=["C2", "C3"], choices=["C2", "C3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("progressive_timing: no GPU (times are measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    this = capi.load_library()
    parent = capi.load_library(os.path.abspath(a.parent)) if a.parent else None
    print(f"this build: {this.pbr_hip_build_info().decode()}", flush=True)
    if parent:
        print(f"parent:     {parent.pbr_hip_build_info().decode()}", flush=True)
    # config -> [(variant, samples per pass, passes per call, calls)]
    plans = {"C2": [("8x8", 8, 8, 1), ("64x1", 1, 64, 1), ("8x8/calls", 8, 1, 8)], "C3": [("4x64", 64, 4, 1)]}
    out = {"rounds": a.rounds, "steps": a.steps, "width": a.width, "height": a.height, "configs": {}}
    for cfg in a.configs:
        scene, rd = scenes.CONFIGS[cfg](a.width, a.height)
        npx = a.width * a.height
        rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
        rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)
        acc = torch.empty((npx, 6), dtype=torch.float32, device=dev)
        variants = ([("plain/parent", None)] if parent else []) + [("plain", None)] + [(p[0], p) for p in plans[cfg]]
        times = {name: [] for name, _ in variants}
        ref = None

        def frame(r, plan):
            if plan is None:
                r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=stream.cuda_stream, sync=False)
                return
            _, per_pass, n_passes, calls = plan
            first = 0
            for _ in range(calls):   # only the last pass of the frame writes an image
                last = first + per_pass * n_passes == HipRenderer.sample_budget(rd)
                r.render_passes(rd, first, per_pass, acc.data_ptr(),
                                [None] * (n_passes - 1) + [rgb.data_ptr() if last else None],
                                [None] * (n_passes - 1) + [rgba.data_ptr() if last else None],
                                stream=stream.cuda_stream)
                first += per_pass * n_passes

        for rnd in range(a.rounds):
            for name, plan in variants:
                # one context at a time (a Path context holds tens of GB of queues)
                r = renderer(parent if name == "plain/parent" else this, scene)
                rgb.fill_(float("nan"))
                frame(r, plan)   # warm-up: code objects, lane buffers
                r.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    frame(r, plan)
                r.sync()
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[name].append(ms)
                img = rgb.cpu().numpy().view(np.uint32)
                if name == "plain":
                    ref = img.copy() if ref is None else ref
                same = ref is None or np.array_equal(img, ref)
                print(f"{cfg} round {rnd} {name:13s} {ms:9.3f} ms{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"{cfg} {name}: the image differs from this build's plain frame")
        res = {}
        for name, _ in variants:
            t = times[name]
            res[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                         "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}
        base = res["plain"]["median_ms"]
        yard = res.get("plain/parent", res["plain"])
        print(f"RESULT {cfg} ({a.width}x{a.height}, {HipRenderer.sample_budget(rd)} spp, {a.rounds} rounds of {a.steps} frames); "
              f"run-to-run spread of {'the parent' if parent else 'this build'}'s plain frame: {100 * yard['spread']:.2f}%")
        for name, _ in variants:
            v = res[name]
            print(f"RESULT {cfg} {name:13s} median {v['median_ms']:9.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}) "
                  f"{100 * (v['median_ms'] / base - 1):+6.2f}% vs plain", flush=True)
        out["configs"][cfg] = res
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
