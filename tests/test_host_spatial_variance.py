"""SamplerIntegrator::Denoise with the spatial variance estimate (DenoiseParams::spatialMinCount of
include/pbr/pbr.h), in a compiled test program (tests/cpp_spatial/spatial_test.cpp): refusals before any device
call; on the GPU, after RenderSamples(0, 1) and RenderFeatures(0, 1) the default parameters still throw and
spatialMinCount = 4 fills the FrameBuffer with the C-ABI result of the same frame, flipped, which this test
computes through the Python layer and hands over in a file."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pysicalbasedraytracer_amd", "host")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp_spatial")], check=True)
    return os.path.join(HERE, "cpp_spatial", "spatial_test")


def _run(args, timeout):
    p = subprocess.run([_build()] + args, capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr


def test_spatial_cpu():
    """spatialMinCount and spatialRadius out of range and missing passes are refused before any device call
    (with or without a GPU: nothing here reaches one)."""
    _run(["cpu"], 120)


@pytest.mark.gpu
def test_spatial_gpu(tmp_path):
    """The compiled program's checks, and its FrameBuffer against pbr_hip_denoise_sv over the passes of the same
    frame: the ball scene of tests/cpp_spatial (a matte sphere of radius 1.5 under a point light, 40×30, Path,
    Halton, the first of 8 samples), min_count 4, radius 1, the default filter parameters."""
    import numpy as np
    import torch
    from pysicalbasedraytracer_amd import HipRenderer, capi, scenes
    s = scenes.Scene()
    s.sphere((0.0, 0.0, 0.0), 1.5, s.matte((0.5, 0.6, 0.7)))
    s.point_light((0.0, 4.0, 4.0), (20.0, 20.0, 20.0))
    rd = scenes.render_desc(scenes.camera(40, 30, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0)), capi.INTEGRATOR_PATH, 8, 8, rr_threshold=0.8)
    dev = torch.device("cuda", 0)
    n = 40 * 30
    acc = torch.zeros((n, 6), dtype=torch.float32, device=dev)
    facc = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    fimg = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    rgba = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    hip = HipRenderer(0)
    try:
        hip.upload(s)
        hip.render_passes(rd, 0, 1, acc.data_ptr(), [None], [None])
        hip.render_aov(rd, 0, 1, facc.data_ptr(), fimg.data_ptr())
        hip.denoise(40, 30, 1, acc.data_ptr(), fimg.data_ptr(), rgb_ptr=rgb.data_ptr(), rgba_ptr=rgba.data_ptr(), spatial=(4, 1))
        hip.sync()
    finally:
        hip.close()
    out, out8 = rgb.cpu().numpy(), rgba.cpu().numpy()
    assert out.dtype == np.float32 and np.isfinite(out).all() and out.max() > 0
    path = tmp_path / "spatial_c_abi.bin"
    with open(path, "wb") as f:
        f.write(out.tobytes())
        f.write(out8.tobytes())
    _run(["gpu", str(path)], 300)
