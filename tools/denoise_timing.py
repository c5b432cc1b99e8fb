"""What the denoiser costs, and that plain frames cost what they did: in ONE process on one GPU.

    python tools/denoise_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

(a) On bench.py's C2 (1920x1080, 64 spp, Halton) and C3 (256 spp, Sobol) scenes every round times, one
after the other, pbr_hip_render of a library built from the parent commit (--parent; skipped without it)
and of this build.  A variant's time is the host clock around `steps` calls queued back to back on one
stream, ending in a synchronise, divided by `steps`.  The rounds alternate the variants, so drift of the
machine reaches both alike; per variant the tool prints median, min and max over the rounds, and the
spread (max - min) / median.  The plain frame of this build must not be slower than the parent's by more
than the larger of the two spreads (the parent is the yardstick); the tool says PASS or FAIL.

(b) pbr_hip_denoise at 1920x1080 and 3840x2160, 5 levels, all three outputs, over a synthetic frame (sky,
a floor with a texture and a distance ramp, a disc with curved normals; 8 gamma-distributed samples per
pixel): median, min and max over the rounds (alternating the two sizes), then from one profiled run the
time of every kernel and, per level, the achieved bytes per second over the level's compulsory traffic —
48 B per pixel: colour/variance and guides read, colour/variance written — beside the 6.29 TB/s a float4
copy measures on this GPU (8.0 TB/s in the specification).  No speed is required of the denoiser."""
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

HBM_COPY_TBS = 6.29   # measured float4 copy on an MI355X; 8.0 TB/s in the specification
LEVEL_BYTES = 48      # per pixel and level: read x/V, read N/z, write x/V
SIZES = ((1920, 1080), (3840, 2160))


def renderer(lib, scene=None):
    capi._lib = lib   # HipRenderer() binds the library loaded last
    r = HipRenderer(0)
    if scene is not None:
        r.upload(scene)
    return r


def synthetic(dev, W, H, samples=8, seed=7):
    """(accum [n, 6], aov [n, 8]) device tensors of a noisy frame: sky above, a checked floor whose distance
    ramps below, a disc with curved normals; every sample is the truth times a gamma variate of mean 1."""
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    floor = yy >= H // 2
    chk = ((torch.div(xx, 16, rounding_mode="floor") + torch.div(yy, 12, rounding_mode="floor")) % 2) > 0
    albedo = torch.zeros((H, W, 3), device=dev)
    albedo[floor & chk] = torch.tensor((0.8, 0.7, 0.2), device=dev)
    albedo[floor & ~chk] = torch.tensor((0.2, 0.3, 0.7), device=dev)
    nrm = torch.zeros((H, W, 3), device=dev)
    nrm[floor] = torch.tensor((0.0, 1.0, 0.0), device=dev)
    dist = torch.where(floor, 2.0 + 10.0 * (H - yy) / H, torch.zeros_like(yy))
    shade = torch.where(floor, 0.5 + 0.5 * (yy - H // 2) / (H - H // 2), torch.ones_like(yy))
    cx, cy, rad = W * 0.55, H * 0.45, min(W, H) * 0.28
    u, v = (xx - cx) / rad, (yy - cy) / rad
    disc = u * u + v * v < 1
    w = torch.sqrt(torch.clamp(1 - u * u - v * v, 0, 1))
    albedo[disc] = torch.tensor((0.9, 0.4, 0.3), device=dev)
    nrm[disc] = torch.stack([u, -v, w], -1)[disc]
    dist = torch.where(disc, 3.0 - w, dist)
    shade = torch.where(disc, 0.2 + 0.8 * w, shade)
    hit = (floor | disc).to(torch.float32)
    sky = torch.tensor((0.3, 0.5, 0.9), device=dev)
    truth = torch.where(hit[..., None] > 0, albedo * shade[..., None], sky.expand(H, W, 3))
    s1 = torch.zeros((H, W, 3), device=dev)
    s2 = torch.zeros((H, W, 3), device=dev)
    gam = torch.distributions.Gamma(torch.tensor(2.0, device=dev), torch.tensor(2.0, device=dev))
    torch.manual_seed(seed)
    for _ in range(samples):
        L = truth * gam.sample((H, W, 1))
        s1 += L
        s2 += L * L
    accum = torch.cat([s1, s2], -1).reshape(-1, 6).contiguous()
    aov = torch.cat([albedo, hit[..., None], nrm, dist[..., None]], -1).reshape(-1, 8).contiguous()
    return accum, aov


def stat(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
            "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}


def plain_frames(a, this, parent, dev, st, say, out):
    """(a): the plain frames of a.configs, this build against the parent's; fills out["configs"] and returns
    whether every plain frame stayed within the bound.  (Shared with tools/temporal_timing.py.)"""
    ok = True
    for cfg in a.configs:
        scene, rd = scenes.CONFIGS[cfg](1920, 1080)
        npx = 1920 * 1080
        rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
        rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)
        names = (["plain/parent"] if parent else []) + ["plain"]
        times = {n: [] for n in names}
        ref = None
        for rnd in range(a.rounds):
            for name in names:
                r = renderer(parent if name == "plain/parent" else this, scene)   # one context at a time
                rgb.fill_(float("nan"))
                torch.cuda.synchronize(dev)
                r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)   # warm-up
                r.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)
                r.sync()
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[name].append(ms)
                bits = rgb.cpu().numpy().view(np.uint32)   # this build computes what the parent computed
                if ref is None:
                    ref = bits.copy()
                same = np.array_equal(bits, ref)
                print(f"{cfg} round {rnd} {name:13s} {ms:10.3f} ms{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"{cfg} {name}: the plain image differs between the builds or the rounds")
        res = {name: stat(times[name]) for name in names}
        say(f"RESULT {cfg} (1920x1080, {HipRenderer.sample_budget(rd)} spp, {a.rounds} rounds of {a.steps} calls)")
        for name in names:
            v = res[name]
            say(f"RESULT {cfg} {name:13s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
                f"spread {100 * v['spread']:.2f}%)")
        if parent:
            p, t = res["plain/parent"], res["plain"]
            slower = t["median_ms"] / p["median_ms"] - 1
            bound = max(p["spread"], t["spread"])
            verdict = "PASS" if slower <= bound else "FAIL"
            ok = ok and slower <= bound
            say(f"RESULT {cfg} (a) plain vs parent: {100 * slower:+.2f}% (bound: the larger spread, {100 * bound:.2f}%) {verdict}")
            res["plain_vs_parent"] = {"slower": slower, "bound": bound, "pass": slower <= bound}
        out["configs"][cfg] = res
        del rgb, rgba
    return ok


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
        sys.exit("denoise_timing: no GPU (times are measured on the device or not at all)")
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
    out = {"rounds": a.rounds, "steps": a.steps, "levels": a.levels, "configs": {}, "denoise": {}}
    # ---- (a) plain frames against the parent's
    ok = plain_frames(a, this, parent, dev, st, say, out)
    # ---- (b) the denoise call
    r = renderer(this)
    frames = {}
    for (W, H) in SIZES:
        acc, aov = synthetic(dev, W, H)
        n = W * H
        frames[W, H] = (acc, aov, torch.empty((n, 3), dtype=torch.float32, device=dev),
                        torch.empty((n, 4), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.float32, device=dev))
    torch.cuda.synchronize(dev)

    def call(W, H):
        acc, aov, rgb, rgba, var = frames[W, H]
        r.denoise(W, H, 8, acc.data_ptr(), aov.data_ptr(), rgb_ptr=rgb.data_ptr(), rgba_ptr=rgba.data_ptr(),
                  var_ptr=var.data_ptr(), iterations=a.levels, stream=st)

    times = {s: [] for s in SIZES}
    for (W, H) in reversed(SIZES):   # (the larger frame first: the planes are allocated once)
        call(W, H)
    r.sync()
    for rnd in range(a.rounds):
        for (W, H) in SIZES:
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(W, H)
            r.sync()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            times[W, H].append(ms)
            print(f"denoise round {rnd} {W}x{H} {ms:10.3f} ms", flush=True)
    for (W, H) in SIZES:
        v = stat(times[W, H])
        n = W * H
        say(f"RESULT denoise {W}x{H}, {a.levels} levels: median {v['median_ms']:.3f} ms (min {v['min_ms']:.3f}, "
            f"max {v['max_ms']:.3f}, spread {100 * v['spread']:.2f}%) = {n / v['median_ms'] / 1e6:.2f} Gpixels/s")
        r.set_profiling(True)
        call(W, H)
        r.sync()
        prof = r.get_profile()
        r.set_profiling(False)
        v["kernels_ms"] = {k: p["ms"] for k, p in prof.items()}
        v["levels"] = []
        say(f"RESULT denoise {W}x{H} profiled: " + ", ".join(f"{k} {p['ms']:.3f} ms" for k, p in prof.items()) +
            f" (sum {sum(p['ms'] for p in prof.values()):.3f} ms)")
        for i in range(a.levels):
            ms = prof[f"k_dn_atrous_l{i}"]["ms"]
            tbs = LEVEL_BYTES * n / (ms * 1e-3) / 1e12
            v["levels"].append({"level": i, "step": 1 << i, "ms": ms, "tb_per_s": tbs, "of_copy_rate": tbs / HBM_COPY_TBS})
            say(f"RESULT denoise {W}x{H} level {i} (step {1 << i:3d}): {ms:.3f} ms, {LEVEL_BYTES} B/pixel compulsory = "
                f"{tbs:.2f} TB/s, {100 * tbs / HBM_COPY_TBS:.0f}% of the {HBM_COPY_TBS} TB/s a float4 copy reaches")
        out["denoise"][f"{W}x{H}"] = v
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# The denoiser: timing\n\n`tools/denoise_timing.py` on one MI355X; every line below is the tool's output.  "
                    "These are the first measurements of these kernels.\n\n```\n" + "\n".join(lines) + "\n```\n")
    if not ok:
        sys.exit("denoise_timing: a plain frame is slower than the parent's by more than the measured spread")


if __name__ == "__main__":
    main()
