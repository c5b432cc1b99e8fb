"""What following mirror bounces in the feature pass costs and buys, and that what existed costs what it did:
in ONE process on one GPU.

    python tools/aov_follow_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

(a) The parent's frames and pass are kept.  On bench.py's C2 (1920x1080, 64 spp) and C3 (256 spp) scenes every
    round times, one after the other, the plain frame of a library built from the parent commit (--parent) and
    of this build, and on C2 the plain feature pass (max_bounces = 0) of both.  A variant's time is the host
    clock around `steps` calls queued back to back on one stream, ending in a synchronise, divided by `steps`;
    the rounds alternate the variants.  The bits of this build must equal the parent's, and its median must
    not be slower than the parent's by more than the larger of the two spreads ((max - min) / median): PASS or
    FAIL, the rule of tools/aov_timing.py.
(b) Cost of following.  The feature pass on C2 at 1920x1080 with mirror_bounces 0, 1 and 4: the HIP-event time
    of the k_aov* families from one profiled call each, and samples per second from the host clock.
(c) What it buys.  C2 at a small size under an 8-frame camera translation: TemporalRender at 2 samples per
    frame, then denoise(spatial=(4, 1)), with mirror_bounces 0 against 4.  The error is the mean squared error
    against a 1024-sample render of the last frame, over the pixels whose first hit is the floor.
No number here is a target: the tool records what comes out."""
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
from pysicalbasedraytracer_amd import HipRenderer, TemporalRender, capi, scenes  # noqa: E402


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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--small", type=int, nargs=2, default=[160, 90], help="the frame of (c)")
    ap.add_argument("--json")
    ap.add_argument("--md", help="write the result lines as a markdown document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aov_follow_timing: no GPU (times are measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    this = capi.load_library()
    parent = capi.load_library(os.path.abspath(a.parent)) if a.parent else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write():   # (after every part, so that a later part's failure leaves the earlier parts' record)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        if a.md:
            with open(a.md, "w") as f:
                f.write("# Following mirror bounces in the feature pass: timing and effect\n\n`tools/aov_follow_timing.py` on one "
                        "MI355X; every line below is the tool's output.\n\n```\n" + "\n".join(lines) + "\n```\n")

    out = {}
    say(f"this build: {this.pbr_hip_build_info().decode()}")
    if parent:
        say(f"parent:     {parent.pbr_hip_build_info().decode()}")
    out.update({"rounds": a.rounds, "steps": a.steps, "width": a.width, "height": a.height, "kept": {}})
    ok = True
    npx = a.width * a.height
    rgb = torch.empty((npx, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((npx, 4), dtype=torch.uint8, device=dev)
    acc = torch.empty((npx, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
    img = torch.empty((npx, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)

    # ---- (a) what existed is kept
    for cfg in ("C2", "C3"):
        scene, rd = scenes.CONFIGS[cfg](a.width, a.height)
        budget = HipRenderer.sample_budget(rd)
        kinds = ["plain"] + (["features"] if cfg == "C2" else [])
        names = [k + sfx for k in kinds for sfx in (["/parent"] if parent else []) + [""]]
        times = {n: [] for n in names}
        ref = {}

        def call(r, name, bounces=0):
            if name.startswith("features"):
                r.render_aov(rd, 0, budget, acc.data_ptr(), img.data_ptr(), stream=st, mirror_bounces=bounces)
            else:
                r.render_device(rd, rgb.data_ptr(), rgba.data_ptr(), stream=st, sync=False)

        for rnd in range(a.rounds):
            for name in names:
                r = renderer(parent if name.endswith("/parent") else this, scene)   # one context at a time
                rgb.fill_(float("nan"))
                img.fill_(float("nan"))
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
                bits = (img if name.startswith("features") else rgb).cpu().numpy().view(np.uint32)
                kind = name.split("/")[0]
                if kind not in ref:
                    ref[kind] = bits.copy()
                same = np.array_equal(bits, ref[kind])
                print(f"{cfg} round {rnd} {name:15s} {ms:10.3f} ms{'' if same else '  IMAGE DIFFERS'}", flush=True)
                r.close()
                if not same:
                    sys.exit(f"{cfg} {name}: the image differs between the builds or the rounds")
        res = {}
        for name in names:
            t = times[name]
            res[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                         "spread": (max(t) - min(t)) / statistics.median(t), "ms": t}
        say(f"RESULT (a) {cfg} ({a.width}x{a.height}, {budget} spp, {a.rounds} rounds of {a.steps} calls)")
        for name in names:
            v = res[name]
            say(f"RESULT (a) {cfg} {name:15s} median {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
                f"spread {100 * v['spread']:.2f}%)")
        if parent:
            for kind in kinds:
                p, t = res[kind + "/parent"], res[kind]
                slower = t["median_ms"] / p["median_ms"] - 1
                bound = max(p["spread"], t["spread"])
                verdict = "PASS" if slower <= bound else "FAIL"
                ok = ok and slower <= bound
                say(f"RESULT (a) {cfg} {kind} vs parent: bits equal, {100 * slower:+.2f}% (bound: the larger spread, "
                    f"{100 * bound:.2f}%) {verdict}")
                res[kind + "_vs_parent"] = {"slower": slower, "bound": bound, "pass": slower <= bound}
        out["kept"][cfg] = res
        write()

    # ---- (b) the cost of following
    scene, rd = scenes.CONFIGS["C2"](a.width, a.height)
    budget = HipRenderer.sample_budget(rd)
    r = renderer(this, scene)
    cost = {}
    for bounces in (0, 1, 4):
        call = lambda: r.render_aov(rd, 0, budget, acc.data_ptr(), img.data_ptr(), stream=st, mirror_bounces=bounces)
        call()
        r.sync()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            r.sync()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
        r.set_profiling(True)
        call()
        r.sync()
        prof = {k: v["ms"] for k, v in r.get_profile().items() if k.startswith("k_aov")}
        r.set_profiling(False)
        ms = statistics.median(ts)
        cost[bounces] = {"median_ms": ms, "ms": ts, "gsamples_per_s": npx * budget / ms / 1e6, "event_ms": prof}
        say(f"RESULT (b) C2 {a.width}x{a.height} {budget} spp mirror_bounces {bounces}: " +
            ", ".join(f"{k} {v:.3f} ms (events)" for k, v in prof.items()) +
            f"; host clock median {ms:.3f} ms = {npx * budget / ms / 1e6:.2f} Gsamples/s")
    r.close()
    out["cost"] = cost
    write()

    # ---- (c) what it buys
    w, h = a.small
    scene, rd = scenes.CONFIGS["C2"](w, h, 32)
    r = renderer(this, scene)
    cams = [scenes.camera(w, h, (0.05 * f, 0.55, 2.6), (0.05 * f, -0.25, 0.0)) for f in range(8)]
    d = type(rd).from_buffer_copy(rd)
    d.camera = cams[-1]
    rd_ref = scenes.render_desc(cams[-1], rd.integrator, 1024, rd.max_depth, rd.rr_threshold, rd.light_strategy, rd.sampler)
    want, _, _ = r.render(rd_ref, rgba=False)
    want = np.asarray(want, dtype=np.float64).reshape(-1, 3)
    facc = torch.zeros((w * h, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
    fimg = torch.zeros((w * h, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    r.render_aov(d, 0, 8, facc.data_ptr(), fimg.data_ptr())
    r.sync()
    first = fimg.cpu().numpy()
    floor = (first[:, 3] == 1) & (first[:, 0] == 1) & (first[:, 2] == 1) & (np.abs(first[:, 5]) == 1)   # Kr = 1, ns = ±y: the mirror floor
    buys = {"floor_pixels": int(floor.sum()), "pixels": w * h}
    for bounces in (0, 4):
        t = TemporalRender(r, rd, 2, cycle=16, mirror_bounces=bounces)
        for cam in cams:
            t.frame(cam)
        got, _ = t.denoise(spatial=(4, 1))
        torch.cuda.synchronize(dev)
        got = got.cpu().numpy().astype(np.float64)
        buys[bounces] = float(((got - want) ** 2)[floor].mean())
    ratio = buys[0] / buys[4] if buys[4] > 0 else float("inf")
    say(f"RESULT (c) C2 {w}x{h}, 8 frames 0.05 apart in x, 2 spp per frame, denoise(spatial=(4, 1)), MSE against 1024 spp over "
        f"the {buys['floor_pixels']} floor pixels: mirror_bounces 0 {buys[0]:.6g}, mirror_bounces 4 {buys[4]:.6g}, ratio {ratio:.3f}")
    buys["ratio"] = ratio
    r.close()
    out["buys"] = {str(k): v for k, v in buys.items()}

    write()
    if not ok:
        sys.exit("aov_follow_timing: something that existed is slower than the parent's by more than the measured spread")


if __name__ == "__main__":
    main()
