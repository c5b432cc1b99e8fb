"""What adaptive sampling costs and saves: listed passes and whole adaptive renders against plain
frames, in ONE process on one GPU.

    python tools/adaptive_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--json out.json]

On bench.py's C3 (1920x1080, 256 spp, Sobol) and C5 (512 spp, Halton) scenes every round times, one
after the other,
  plain/parent   pbr_hip_render of a library built from the parent commit (--parent; skipped without it)
  plain          pbr_hip_render of this build
  uniform        one pbr_hip_render_passes pass of the whole budget
  listed/all     the same pass through pbr_hip_render_passes_list with every pixel listed: what the list
                 machinery (run encoding and its readback, gather, the tile search over runs, scatter) costs
  min pass       one uniform pass of --min-samples samples (the first step of an adaptive render)
  select         pbr_hip_adaptive_select over every pixel of that pass's sums, alone
  adaptive       pbr_hip_render_adaptive at --tolerance (0.02), --min-samples, --per-round
A variant's time is the host clock around `steps` calls queued back to back on one stream, ending in a
synchronise, divided by `steps`.  The rounds alternate the variants, so drift of the machine reaches
all of them alike; per variant the tool prints median, min and max over the rounds, and the spread
(max - min) / median.  uniform and listed/all must leave the plain frame bit for bit.  For adaptive the
tool reports the samples taken, the rounds, and the samples per second of the active rounds:
(samples - pixels x min_samples) / (adaptive - min pass), next to the plain frame's samples per second."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--configs", nargs="+", default=["C3", "C5"], choices=["C2", "C3", "C5"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=0, help="the budget (0: the config's benchmark budget)")
    ap.add_argument("--tolerance", type=float, default=0.02)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--per-round", type=int, default=16)
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adaptive_timing: no GPU (times are measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    this = capi.load_library()
    parent = capi.load_library(os.path.abspath(a.parent)) if a.parent else None
    print(f"this build: {this.pbr_hip_build_info().decode()}", flush=True)
    if parent:
        print(f"parent:     {parent.pbr_hip_build_info().decode()}", flush=True)
    out = {"rounds": a.rounds, "steps": a.steps, "width": a.width, "height": a.height, "tolerance": a.tolerance,
           "floor": a.floor, "min_samples": a.min_samples, "per_round": a.per_round, "configs": {}}
    for cfg in a.configs:
        scene, rd = scenes.CONFIGS[cfg](a.width, a.height, a.spp) if a.spp else scenes.CONFIGS[cfg](a.width, a.height)
        npx = a.width * a.height
        budget = HipRenderer.sample_budget(rd)
        rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
        rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)
        acc = torch.empty((npx, 6), dtype=torch.float32, device=dev)
        counts = torch.empty((npx,), dtype=torch.int32, device=dev)
        every = torch.arange(npx, dtype=torch.int32, device=dev)
        scratch = torch.empty((npx,), dtype=torch.int32, device=dev)
        names = (["plain/parent"] if parent else []) + ["plain", "uniform", "listed/all", "min pass", "select", "adaptive"]
        times = {n: [] for n in names}
        ref, adaptive_res = None, None
        st = stream.cuda_stream

        def call(r, name):
            if name in ("plain", "plain/parent"):
                r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)
            elif name == "uniform":
                r.render_passes(rd, 0, budget, acc.data_ptr(), [rgb.data_ptr()], [rgba.data_ptr()], stream=st)
            elif name == "listed/all":
                r.render_passes_list(rd, 0, budget, every.data_ptr(), npx, acc.data_ptr(), rgb.data_ptr(), rgba.data_ptr(), stream=st)
            elif name == "min pass":
                r.render_passes(rd, 0, a.min_samples, acc.data_ptr(), [rgb.data_ptr()], [rgba.data_ptr()], stream=st)
            elif name == "select":   # (over the sums the warm-up's min pass left)
                r.adaptive_select(npx, a.min_samples, a.tolerance, a.floor, acc.data_ptr(), scratch.data_ptr())
            else:
                return r.render_adaptive(rd, a.min_samples, a.per_round, a.tolerance, a.floor, acc.data_ptr(), counts.data_ptr(),
                                         rgb.data_ptr(), rgba.data_ptr(), stream=st)

        for rnd in range(a.rounds):
            for name in names:
                # one context at a time (a Path context holds tens of GB of queues)
                r = renderer(parent if name == "plain/parent" else this, scene)
                rgb.fill_(float("nan"))
                torch.cuda.synchronize(dev)
                call(r, "min pass" if name == "select" else name)   # warm-up: code objects, lane buffers
                r.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    res = call(r, name)
                r.sync()
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[name].append(ms)
                same = True
                if name in ("plain", "uniform", "listed/all"):
                    img = rgb.cpu().numpy().view(np.uint32)
                    if name == "plain" and ref is None:
                        ref = img.copy()
                    same = np.array_equal(img, ref)
                note = ""
                if name == "adaptive":
                    c = counts.cpu().numpy()
                    adaptive_res = {"samples": int(res.samples), "rounds": int(res.rounds), "max_samples_done": int(res.max_samples_done),
                                    "active_at_end": int(res.active_at_end), "mean_spp": float(c.mean()),
                                    "pixels_at_min": int((c == a.min_samples).sum()), "pixels_at_budget": int((c == budget).sum())}
                    assert int(c.sum()) == res.samples
                    note = f"  {res.samples / (npx * budget):.3f} of the plain frame's samples, {res.rounds} passes"
                print(f"{cfg} round {rnd} {name:13s} {ms:10.3f} ms{note}{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"{cfg} {name}: the image differs from this build's plain frame")
        res = {}
        for name in names:
            t = times[name]
            res[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                         "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}
        base = res["plain"]["median_ms"]
        print(f"RESULT {cfg} ({a.width}x{a.height}, budget {budget} spp, {a.rounds} rounds of {a.steps} calls)")
        for name in names:
            v = res[name]
            print(f"RESULT {cfg} {name:13s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
                  f"spread {100 * v['spread']:.2f}%) {100 * (v['median_ms'] / base - 1):+7.2f}% vs plain", flush=True)
        listed, uniform = res["listed/all"]["median_ms"], res["uniform"]["median_ms"]
        print(f"RESULT {cfg} (a) listed/all - uniform = {listed - uniform:+.3f} ms ({100 * (listed / uniform - 1):+.2f}%); "
              f"spreads {100 * res['uniform']['spread']:.2f}% / {100 * res['listed/all']['spread']:.2f}%")
        active_s = (res["adaptive"]["median_ms"] - res["min pass"]["median_ms"]) / 1e3
        extra = adaptive_res["samples"] - npx * a.min_samples
        adaptive_res["active_rounds_samples_per_s"] = extra / active_s if active_s > 0 and extra > 0 else None
        adaptive_res["plain_samples_per_s"] = npx * budget / (base / 1e3)
        print(f"RESULT {cfg} (b) adaptive at tolerance {a.tolerance}: {adaptive_res['samples']} samples "
              f"({adaptive_res['samples'] / (npx * budget):.3f} of plain, mean {adaptive_res['mean_spp']:.1f} spp, "
              f"{adaptive_res['pixels_at_min']} pixels at {a.min_samples}, {adaptive_res['pixels_at_budget']} at the budget), "
              f"{adaptive_res['rounds']} passes, {res['adaptive']['median_ms']:.1f} ms vs plain {base:.1f} ms; active rounds "
              f"{(adaptive_res['active_rounds_samples_per_s'] or 0) / 1e6:.1f} Msamples/s vs plain "
              f"{adaptive_res['plain_samples_per_s'] / 1e6:.1f}", flush=True)
        res["adaptive_result"] = adaptive_res
        out["configs"][cfg] = res
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
