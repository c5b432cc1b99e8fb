"""What feature buffers cost, and that plain frames cost what they did: in ONE process on one GPU.

    python tools/aov_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

On bench.py's C2 (1920x1080, 64 spp, Halton) and C3 (256 spp, Sobol) scenes every round times, one after
the other,
  plain/parent   pbr_hip_render of a library built from the parent commit (--parent; skipped without it)
  plain          pbr_hip_render of this build
  features/parent  the same feature pass of the parent's library (--parent; skipped without it)
  features       one pbr_hip_render_aov pass over the frame's full sample count, image included
A variant's time is the host clock around `steps` calls queued back to back on one stream, ending in a
synchronise, divided by `steps`.  The rounds alternate the variants, so drift of the machine reaches all
of them alike; per variant the tool prints median, min and max over the rounds, and the spread
(max - min) / median.  (a) The plain frame of this build must not be slower than the parent's by more
than the larger of the two spreads (the parent is the yardstick); the tool says PASS or FAIL.  (b) No
speed is required of the feature pass; it is reported beside the time of the nearest existing kernel,
the camera kernel of the plain frame (k_wfp_camera_extend for Path), from one profiled run of each."""
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

CAMERA_KERNELS = ("k_wfp_camera_extend", "k_wf_camera_extend", "k_wf_shade_l0")


def renderer(lib, scene):
    capi._lib = lib   # HipRenderer() binds the library loaded last
    r = HipRenderer(0)
    r.upload(scene)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libpbr_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--configs", nargs="+", default=["C2", "C3"], choices=["C2", "C3", "C5"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=0, help="the budget (0: the config's benchmark budget)")
    ap.add_argument("--normals", action="store_true",
                    help="the scenes on the stand-in mesh carrying its analytic per-vertex normals")
    ap.add_argument("--json")
    ap.add_argument("--md", help="write the result lines as a markdown document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aov_timing: no GPU (times are measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    this = capi.load_library()
    parent = capi.load_library(os.path.abspath(a.parent)) if a.parent else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"this build: {this.pbr_hip_build_info().decode()}")
    if parent:
        say(f"parent:     {parent.pbr_hip_build_info().decode()}")
    out = {"rounds": a.rounds, "steps": a.steps, "width": a.width, "height": a.height, "configs": {}}
    ok = True
    for cfg in a.configs:
        size = (a.width, a.height, a.spp) if a.spp else (a.width, a.height)
        if a.normals:   # the kernels' NRM instantiations (k_aov<true, ...>, k_wf_shade<true, ...>)
            P, I, N = scenes.dragon_standin(normals=True)
            scene, rd = scenes.CONFIGS[cfg](*size, mesh=(P, I, "standin:displaced-uv-sphere-224"))
            scene.shapes[0].N = capi.fptr(N)
            scene._keep.append(N)
        else:
            scene, rd = scenes.CONFIGS[cfg](*size)
        npx = a.width * a.height
        budget = HipRenderer.sample_budget(rd)
        rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
        rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)
        acc = torch.empty((npx, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
        img = torch.empty((npx, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
        names = (["plain/parent"] if parent else []) + ["plain"] + (["features/parent"] if parent else []) + ["features"]
        times = {n: [] for n in names}
        ref = ref_feat = None
        st = stream.cuda_stream

        def call(r, name):
            if name.startswith("features"):
                r.render_aov(rd, 0, budget, acc.data_ptr(), img.data_ptr(), stream=st)
            else:
                r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)

        for rnd in range(a.rounds):
            for name in names:
                r = renderer(parent if name.endswith("/parent") else this, scene)   # one context at a time
                rgb.fill_(float("nan"))
                torch.cuda.synchronize(dev)
                call(r, name)   # warm-up: code objects, lane buffers
                r.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(r, name)
                r.sync()
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[name].append(ms)
                same = True
                if name.startswith("features"):   # this build computes what the parent computed
                    bits = img.cpu().numpy().view(np.uint32)
                    if ref_feat is None:
                        ref_feat = bits.copy()
                    same = np.array_equal(bits, ref_feat)
                else:
                    bits = rgb.cpu().numpy().view(np.uint32)
                    if ref is None:
                        ref = bits.copy()
                    same = np.array_equal(bits, ref)
                print(f"{cfg} round {rnd} {name:15s} {ms:10.3f} ms{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"{cfg} {name}: the image differs between the builds or the rounds")
        res = {}
        for name in names:
            t = times[name]
            res[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                         "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}
        say(f"RESULT {cfg} ({a.width}x{a.height}, {budget} spp, {a.rounds} rounds of {a.steps} calls{', per-vertex normals' if a.normals else ''})")
        for name in names:
            v = res[name]
            say(f"RESULT {cfg} {name:15s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
                f"spread {100 * v['spread']:.2f}%)")
        if parent:
            p, t = res["plain/parent"], res["plain"]
            slower = t["median_ms"] / p["median_ms"] - 1
            bound = max(p["spread"], t["spread"])
            verdict = "PASS" if slower <= bound else "FAIL"
            ok = ok and slower <= bound
            say(f"RESULT {cfg} (a) plain vs parent: {100 * slower:+.2f}% (bound: the larger spread, {100 * bound:.2f}%) {verdict}")
            res["plain_vs_parent"] = {"slower": slower, "bound": bound, "pass": slower <= bound}
            p, t = res["features/parent"], res["features"]   # reported; no speed is required of the pass
            say(f"RESULT {cfg} features vs parent: {100 * (t['median_ms'] / p['median_ms'] - 1):+.2f}% "
                f"(the larger spread: {100 * max(p['spread'], t['spread']):.2f}%)")
        # (b) one profiled run of each: the feature kernel beside the plain frame's camera kernel
        r = renderer(this, scene)
        r.set_profiling(True)
        call(r, "plain")
        r.sync()
        plain_prof = r.get_profile()
        call(r, "features")
        r.sync()
        feat_prof = r.get_profile()
        r.set_profiling(False)
        r.close()
        cams = {k: plain_prof[k]["ms"] for k in CAMERA_KERNELS if k in plain_prof}
        feats = {k: v["ms"] for k, v in feat_prof.items() if k.startswith("k_aov")}
        f = res["features"]["median_ms"]
        say(f"RESULT {cfg} (b) features {f:.3f} ms = {npx * budget / f / 1e6:.1f} Gsamples/s, "
            f"{100 * f / res['plain']['median_ms']:.1f}% of the plain frame; profiled: " +
            ", ".join(f"{k} {v:.3f} ms" for k, v in feats.items()) + " beside the plain frame's " +
            (", ".join(f"{k} {v:.3f} ms" for k, v in cams.items()) or "camera kernel (none profiled)"))
        res["profile"] = {"features": feats, "camera": cams}
        out["configs"][cfg] = res
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Feature passes: timing\n\n`tools/aov_timing.py` on one MI355X; every line below is the tool's output.\n\n```\n" +
                    "\n".join(lines) + "\n```\n")
    if not ok:
        sys.exit("aov_timing: a plain frame is slower than the parent's by more than the measured spread")


if __name__ == "__main__":
    main()
