"""What temporal accumulation costs, and that plain frames cost what they did: in ONE process on one GPU.

    python tools/temporal_timing.py --parent path/to/parent/libpbr_hip.so [--rounds 5] [--steps 2] [--md out.md] [--json out.json]

(a) The plain C2 and C3 frames of this build against a library built from the parent commit, by
tools/denoise_timing.py's own procedure and rule (same bits; not slower than the parent's by more than
the larger of the two measured spreads); the tool says PASS or FAIL.

(b) pbr_hip_temporal at 1920x1080 and 3840x2160, every output asked for, over a synthetic moving-camera
pair (tests/temporal_expected.py's world — a checkered floor, a wall, a sphere, sky — 4 gamma-distributed
samples per pixel, the camera panning 0.2 units between the frames): median, min and max over the rounds
(alternating the two sizes; a time is the host clock around `steps` calls queued back to back on one
stream, ending in a synchronise, divided by `steps`), then from one profiled run the kernel's time and
the achieved bytes per second over the call's compulsory traffic — 168 B per pixel: this frame's sums and
features read (56), the previous frame's sums, features and counts read once (60), sums and counts
written (28), motion, rgb and rgba written (24), and 4 more where per-pixel counts are read (not here) —
beside the 6.29 TB/s a float4 copy measures on this GPU (8.0 TB/s in the specification).  The same call
with the previous camera turned round — no pixel projects, no tap is read: 108 B per pixel streamed — is
timed beside it, to tell the streaming part from the four gathers.  No speed is required of the call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_expected as TE  # noqa: E402
from denoise_timing import HBM_COPY_TBS, SIZES, plain_frames, renderer, stat  # noqa: E402
from pysicalbasedraytracer_amd import capi  # noqa: E402

CALL_BYTES = 56 + 60 + 28 + 24   # per pixel, every output asked for, no per-pixel current counts
STREAM_BYTES = 56 + 28 + 24      # ... when no pixel projects into the previous frame: no tap is read
SAMPLES = 4


def moving_pair(dev, W, H):
    """Device tensors and matrices of two frames of the synthetic world, the camera panned 0.2 units."""
    cams = TE.camera(W, H, eye=(0.2, 0.5, 2.0), look=(0.2, 0.0, -4.0)), TE.camera(W, H)
    cur = TE.synthetic_frame(cams[0], SAMPLES, seed=1)
    prev = TE.synthetic_frame(cams[1], SAMPLES, seed=2)
    up = lambda a: torch.from_numpy(a).to(dev)
    n = W * H
    return dict(accum_cur=up(cur[0]), aov_cur=up(cur[1]), accum_prev=up(prev[0]), aov_prev=up(prev[1]),
                counts_prev=torch.full((n,), SAMPLES, dtype=torch.int32, device=dev), cur=cur[3], prev=prev[3],
                accum_out=torch.empty((n, 6), dtype=torch.float32, device=dev), counts_out=torch.empty((n,), dtype=torch.int32, device=dev),
                motion=torch.empty((n, 2), dtype=torch.float32, device=dev), rgb=torch.empty((n, 3), dtype=torch.float32, device=dev),
                rgba=torch.empty((n, 4), dtype=torch.uint8, device=dev), hit=int((cur[1][:, 3] > 0).sum()),
                away=capi.camera_matrices(TE.previous_camera(W, H, "turned_round")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libpbr_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--configs", nargs="*", default=["C2", "C3"], choices=["C2", "C3", "C5"])
    ap.add_argument("--json")
    ap.add_argument("--md", help="write the result lines as a markdown document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("temporal_timing: no GPU (times are measured on the device or not at all)")
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
    out = {"rounds": a.rounds, "steps": a.steps, "configs": {}, "temporal": {}}
    # ---- (a) plain frames against the parent's
    ok = plain_frames(a, this, parent, dev, st, say, out)
    # ---- (b) the temporal call
    r = renderer(this)
    frames = {s: moving_pair(dev, *s) for s in SIZES}
    torch.cuda.synchronize(dev)

    def call(W, H, away=False):
        f = frames[W, H]
        r.temporal(W, H, SAMPLES, f["accum_cur"].data_ptr(), f["aov_cur"].data_ptr(), f["counts_prev"].data_ptr(),
                   f["accum_prev"].data_ptr(), f["aov_prev"].data_ptr(), f["accum_out"].data_ptr(), f["counts_out"].data_ptr(),
                   f["cur"], f["away" if away else "prev"], motion_ptr=f["motion"].data_ptr(), rgb_ptr=f["rgb"].data_ptr(), rgba_ptr=f["rgba"].data_ptr(),
                   stream=st)

    times = {(s, away): [] for s in SIZES for away in (False, True)}
    for (W, H) in SIZES:   # warm-up
        call(W, H)
    r.sync()
    for rnd in range(a.rounds):
        for (W, H) in SIZES:
            for away in (True, False):   # (the merged frame is the one left in the outputs)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(W, H, away)
                r.sync()
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[(W, H), away].append(ms)
                print(f"temporal round {rnd} {W}x{H}{' no projection' if away else ''} {ms:10.3f} ms", flush=True)
    for (W, H) in SIZES:
        v = stat(times[(W, H), False])
        n = W * H
        took = int((frames[W, H]["counts_out"] > SAMPLES).sum())
        say(f"RESULT temporal {W}x{H}: median {v['median_ms']:.3f} ms (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, "
            f"spread {100 * v['spread']:.2f}%) = {n / v['median_ms'] / 1e6:.2f} Gpixels/s; {took} of {frames[W, H]['hit']} hit "
            f"pixels take history")
        r.set_profiling(True)
        call(W, H)
        r.sync()
        prof = r.get_profile()
        r.set_profiling(False)
        ms = prof["k_tp_accumulate"]["ms"]
        tbs = CALL_BYTES * n / (ms * 1e-3) / 1e12
        v.update(kernel_ms=ms, launches=prof["k_tp_accumulate"]["launches"], bytes_per_pixel=CALL_BYTES, tb_per_s=tbs,
                 of_copy_rate=tbs / HBM_COPY_TBS, took_history=took, hit=frames[W, H]["hit"])
        say(f"RESULT temporal {W}x{H} profiled: k_tp_accumulate {ms:.3f} ms in {prof['k_tp_accumulate']['launches']} launch, "
            f"{CALL_BYTES} B/pixel compulsory = {tbs:.2f} TB/s, {100 * tbs / HBM_COPY_TBS:.0f}% of the {HBM_COPY_TBS} TB/s a float4 "
            f"copy reaches")
        r.set_profiling(True)
        call(W, H, away=True)
        r.sync()
        ms = r.get_profile()["k_tp_accumulate"]["ms"]
        r.set_profiling(False)
        w = stat(times[(W, H), True])
        tbs = STREAM_BYTES * n / (ms * 1e-3) / 1e12
        w.update(kernel_ms=ms, bytes_per_pixel=STREAM_BYTES, tb_per_s=tbs, of_copy_rate=tbs / HBM_COPY_TBS)
        v["no_projection"] = w
        say(f"RESULT temporal {W}x{H} with no pixel projecting (no tap read): median {w['median_ms']:.3f} ms (spread "
            f"{100 * w['spread']:.2f}%); profiled {ms:.3f} ms, {STREAM_BYTES} B/pixel = {tbs:.2f} TB/s, "
            f"{100 * tbs / HBM_COPY_TBS:.0f}% of the copy rate")
        out["temporal"][f"{W}x{H}"] = v
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Temporal accumulation: timing\n\n`tools/temporal_timing.py` on one MI355X; every line below is the tool's "
                    "output.  These are the first measurements of this kernel.\n\n```\n" + "\n".join(lines) + "\n```\n")
    if not ok:
        sys.exit("temporal_timing: a plain frame is slower than the parent's by more than the measured spread")


if __name__ == "__main__":
    main()
