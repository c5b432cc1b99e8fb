"""What per-vertex shading normals cost, and that scenes without them cost what they did: in ONE process
on one GPU.

    python tools/shading_normals_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

(a) On bench.py's C2 (1920x1080, 64 spp, Halton) and C3 (256 spp, Sobol) scenes, which have no normals,
every round times pbr_hip_render of a library built from the parent commit (--parent) and of this build,
one after the other.  A time is the host clock around `steps` calls queued back to back on one stream,
ending in a synchronise, divided by `steps`.  The rounds alternate the two builds, so drift of the
machine reaches both alike.  The parent's rounds against each other are the yardstick: this build passes
if its median is no higher than the parent's slowest round; the tool says PASS or FAIL, and checks that
both builds render the same bits.

(b) The C2 frame with the stand-in mesh carrying its analytic normals (dragon_standin(normals=True))
against the same mesh flat, this build only, alternating as above.  The cost of normals is reported, not
gated, with the shading kernels' profiled times of one run of each."""
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


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
            "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}


def c2_standin(width, height, spp, normals):
    """bench.py's C2 scene on the stand-in mesh, with or without its analytic normals."""
    P, I, N = scenes.dragon_standin(normals=True)
    s, rd = scenes.config_c2(width, height, spp, mesh=(P, I, "standin:displaced-uv-sphere-224"))
    if normals:
        s.shapes[0].N = capi.fptr(N)
        s._keep.append(N)
    return s, rd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libpbr_hip.so built from the parent commit (without it, (a) is skipped)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--configs", nargs="+", default=["C2", "C3"], choices=["C2", "C3", "C5"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=0, help="the budget (0: the config's benchmark budget)")
    ap.add_argument("--json")
    ap.add_argument("--md", help="write the result lines as a markdown document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shading_normals_timing: no GPU (times are measured on the device or not at all)")
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
    npx = a.width * a.height
    rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)

    def timed(lib, scene, rd):
        """(ms per frame, the frame's bits) of `steps` frames after one warm-up frame, on a fresh context."""
        r = renderer(lib, scene)
        rgb.fill_(float("nan"))
        torch.cuda.synchronize(dev)
        r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)   # warm-up: code objects, lane buffers
        r.sync()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)
        r.sync()
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        bits = rgb.cpu().numpy().view(np.uint32).copy()
        r.close()
        return ms, bits

    out = {"rounds": a.rounds, "steps": a.steps, "width": a.width, "height": a.height, "no_normals": {}}
    ok = True
    # ---- (a) scenes without normals: this build against the parent
    for cfg in a.configs if parent else []:
        scene, rd = scenes.CONFIGS[cfg](a.width, a.height, a.spp) if a.spp else scenes.CONFIGS[cfg](a.width, a.height)
        times, ref = {"parent": [], "this": []}, None
        for rnd in range(a.rounds):
            for name, lib in (("parent", parent), ("this", this)):
                ms, bits = timed(lib, scene, rd)
                times[name].append(ms)
                if ref is None:
                    ref = bits
                print(f"{cfg} round {rnd} {name:7s} {ms:10.3f} ms", flush=True)
                if not np.array_equal(bits, ref):
                    sys.exit(f"{cfg} {name}: the image differs between the builds or the rounds")
        res = {k: stats(v) for k, v in times.items()}
        say(f"RESULT {cfg} ({a.width}x{a.height}, {HipRenderer.sample_budget(rd)} spp, {a.rounds} rounds of {a.steps} frames, same bits)")
        for name in ("parent", "this"):
            v = res[name]
            say(f"RESULT {cfg} {name:7s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
                f"spread {100 * v['spread']:.2f}%)")
        p, t = res["parent"], res["this"]
        passed = t["median_ms"] <= p["max_ms"]
        ok = ok and passed
        say(f"RESULT {cfg} (a) no normals: this build {100 * (t['median_ms'] / p['median_ms'] - 1):+.2f}% of the parent's median; "
            f"the parent's own rounds span {p['min_ms']:.3f}..{p['max_ms']:.3f} ms: {'PASS' if passed else 'FAIL'}")
        res["pass"] = passed
        out["no_normals"][cfg] = res
    # ---- (b) what the normals cost: C2 on the stand-in mesh, smooth against flat
    spp = a.spp or 64
    variants = {"flat": c2_standin(a.width, a.height, spp, False), "normals": c2_standin(a.width, a.height, spp, True)}
    times = {k: [] for k in variants}
    for rnd in range(a.rounds):
        for name, (scene, rd) in variants.items():
            ms, _ = timed(this, scene, rd)
            times[name].append(ms)
            print(f"C2/standin round {rnd} {name:7s} {ms:10.3f} ms", flush=True)
    res = {k: stats(v) for k, v in times.items()}
    prof = {}
    for name, (scene, rd) in variants.items():   # one profiled frame of each
        r = renderer(this, scene)
        r.set_profiling(True)
        r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)
        r.sync()
        prof[name] = {k: v["ms"] for k, v in r.get_profile().items()}
        r.set_profiling(False)
        r.close()
    say(f"RESULT C2/standin ({a.width}x{a.height}, {spp} spp, 100,352 triangles, {a.rounds} rounds of {a.steps} frames)")
    for name in variants:
        v = res[name]
        say(f"RESULT C2/standin {name:7s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
            f"spread {100 * v['spread']:.2f}%)")
    say(f"RESULT C2/standin (b) normals cost {100 * (res['normals']['median_ms'] / res['flat']['median_ms'] - 1):+.2f}% of the flat frame "
        f"(a smooth-shaded frame is another image: other bounce directions); profiled kernels, flat -> normals: " +
        ", ".join(f"{k} {prof['flat'].get(k, 0.0):.3f} -> {prof['normals'].get(k, 0.0):.3f} ms" for k in sorted(prof["normals"])))
    res["profile"] = prof
    out["normals_cost"] = res
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Shading normals: timing\n\n`tools/shading_normals_timing.py` on one MI355X; every line below is the tool's "
                    "output.\n\n```\n" + "\n".join(lines) + "\n```\n")
    if not ok:
        sys.exit("shading_normals_timing: a frame without normals is slower than the parent's slowest round")


if __name__ == "__main__":
    main()
