"""bench.py's command line: a plain run times the frames and prints the headline line only; the
roofline, SURVEY-model and CPU-baseline legs sit behind --full; --dump-outputs writes the last timed
frame as float32 .npy within 64 MB, a fixed seeded pixel sample where the frame is larger."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

LIMIT = 64 * 10 ** 6


def test_dump_sample_keeps_a_frame_that_fits_whole():
    assert bench.dump_pixel_sample(1920 * 1080) is None          # C2, C3, C5: 28 B a pixel = 58 MB
    assert 1920 * 1080 * 28 <= LIMIT


def test_dump_sample_of_a_larger_frame_is_fixed_and_fits():
    n = 3840 * 2160                                               # C4
    a, b = bench.dump_pixel_sample(n), bench.dump_pixel_sample(n)
    assert a.dtype == np.int64 and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < n     # sorted, distinct, inside the frame
    assert a.size * (12 + 16 + 8) <= LIMIT and a.size >= n // 8   # rgb + rgba8 + index, a dense sample
    # just over the budget: still a sample, never more pixels than the frame has
    m = bench.DUMP_BUDGET_BYTES // 28 + 1
    s = bench.dump_pixel_sample(m)
    assert s is not None and s.size < m and s[-1] < m


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_frame(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert "Msamples/sec" in d["metric"]
    # value and ms_per_step are one measurement: C2's 1920 x 1080 x 64 samples per step
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1920 * 1080 * 64 / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    # the legs that take runs of their own are --full's
    assert "roofline" not in d and "cpu_baseline" not in d and "gpu_over_cpu" not in d
    # the stderr progress shows one timed window of 2 frames and no other
    windows = [ln for ln in p.stderr.splitlines() if ln.startswith("[bench]")]
    assert len(windows) == 1 and " 2 frame(s) " in windows[0], windows
    rgb, rgba = np.load(out / "rgb.npy"), np.load(out / "rgba8.npy")
    assert sorted(os.listdir(out)) == ["rgb.npy", "rgba8.npy"]
    assert rgb.dtype == np.float32 and rgb.shape == (1920 * 1080, 3)
    assert rgba.dtype == np.float32 and rgba.shape == (1920 * 1080, 4)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= LIMIT
    assert np.isfinite(rgb).all() and (rgb >= 0).all() and rgb.max() > 0
    assert np.array_equal(rgba, np.round(rgba)) and rgba.min() >= 0 and rgba.max() <= 255 and rgba.max() > 0
