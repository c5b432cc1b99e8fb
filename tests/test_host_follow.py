"""SamplerIntegrator::RenderFeatures(..., mirrorBounces) of the C++ host API (include/pbr/pbr.h), in a
compiled test program (tests/cpp_follow/follow_test.cpp): an out-of-range value throws before any device
call; on the GPU the default argument is the plain pass, and the buffers with 0 and 2 bounces equal the C-ABI
images of the same frame, which this test renders through the Python layer and hands over in files."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pysicalbasedraytracer_amd", "host")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp_follow")], check=True)
    return os.path.join(HERE, "cpp_follow", "follow_test")


def _run(args, timeout):
    p = subprocess.run([_build()] + args, capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr


def test_mirror_bounces_out_of_range_throw_before_any_device_call():
    """With or without a GPU: the refusal comes first, so no device is asked for."""
    _run(["cpu"], 120)


@pytest.mark.gpu
def test_render_features_follows_mirrors(tmp_path):
    """The compiled program's checks, and its buffers against pbr_hip_render_aov_mirrors' images of the same
    frame: two mirror balls either side of a matte one (radius 1.5, x = -3.25, 0, 3.25), 40×30, Halton, 8 spp."""
    import numpy as np
    import torch
    from pysicalbasedraytracer_amd import HipRenderer, capi, scenes
    s = scenes.Scene()
    s.sphere((0.0, 0.0, 0.0), 1.5, s.matte((0.5, 0.75, 0.25)))
    s.sphere((-3.25, 0.0, 0.0), 1.5, s.mirror((0.5, 1.0, 0.25)))
    s.sphere((3.25, 0.0, 0.0), 1.5, s.mirror((1.0, 0.5, 0.5)))
    s.point_light((0.0, 4.0, 4.0), (20.0, 20.0, 20.0))
    rd = scenes.render_desc(scenes.camera(40, 30, (0.0, 0.0, 7.0), (0.0, 0.0, 0.0)), capi.INTEGRATOR_PATH, 8, 8, rr_threshold=0.8)
    dev = torch.device("cuda", 0)
    paths = []
    hip = HipRenderer(0)
    try:
        hip.upload(s)
        for bounces in (0, 2):
            acc = torch.zeros((40 * 30, 8), dtype=torch.float32, device=dev)
            img = torch.zeros((40 * 30, 8), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            hip.render_aov(rd, 0, 8, acc.data_ptr(), img.data_ptr(), mirror_bounces=bounces)
            hip.sync()
            out = img.cpu().numpy()
            assert out.dtype == np.float32 and 0 < out[:, 3].sum() < 40 * 30
            paths.append(tmp_path / f"aov_c_abi_{bounces}.f32")
            out.tofile(paths[-1])
    finally:
        hip.close()
    _run(["gpu"] + [str(p) for p in paths], 300)
