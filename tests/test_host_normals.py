"""A TriangleMesh with per-vertex normals through the C++ host API (include/pbr/pbr.h), in a compiled test
program (tests/cpp_normals/normals_test.cpp): the mesh uploads and renders, and Scene::Intersect's
SurfaceInteraction (n, shading.n, shading.dpdu) equals pbr_hip_query's records of the same scene built
through the Python layer, which this test hands over in a file."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the tent mesh of normals_test.cpp
P = [(-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.5, -1.0), (-1.0, 0.25, -1.0)]
I = [(0, 1, 2), (0, 2, 3)]
N = [(-0.25, 1.0, 0.25), (0.25, 1.0, 0.25), (0.25, 1.0, -0.125), (-0.25, 1.0, -0.25)]


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pysicalbasedraytracer_amd", "host")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp_normals")], check=True)
    return os.path.join(HERE, "cpp_normals", "normals_test")


def test_the_program_builds():
    assert os.access(_build(), os.X_OK)


@pytest.mark.gpu
def test_host_mesh_normals_gpu(tmp_path):
    import ctypes as C

    import numpy as np
    from pysicalbasedraytracer_amd import HipRenderer, capi, scenes
    s = scenes.Scene()
    xf = scenes.compose(scenes.translate(0.25, -0.5, 0.0), scenes.scale(2.0, 1.0, 0.5))
    s.mesh(np.array(P, np.float32), np.array(I, np.int32), s.matte((0.6, 0.6, 0.6)), xform=xf, normals=np.array(N, np.float32))
    s.point_light((0.0, 4.0, 2.0), (20.0, 20.0, 20.0))
    rng = np.random.default_rng(5)
    rays = np.zeros((40, 7), dtype=np.float32)
    rays[:, 0] = rng.uniform(-1.6, 2.1, 40)
    rays[:, 1] = 3.0
    rays[:, 2] = rng.uniform(-0.45, 0.45, 40)
    rays[:20, 4] = -1.0                                   # straight down …
    rays[20:, 3:6] = rng.normal(0, 0.2, (20, 3)) + (0, -1, 0)   # … and slanted
    rays[:, 6] = np.inf
    hip = HipRenderer(0)
    try:
        hip.upload(s)
        out = (capi.SurfaceHit * 40)()
        hip._check(hip.lib.pbr_hip_query(hip.ctx, 40, capi.fptr(rays), 0, -1, out), "query")
    finally:
        hip.close()
    assert C.sizeof(capi.SurfaceHit) == 112
    w = np.frombuffer(out, dtype=np.float32).reshape(40, 28)
    assert (w.view(np.int32)[:, 0] == 1).sum() >= 20
    rec = np.concatenate([rays, w[:, 12:21]], axis=1).astype(np.float32)
    path = tmp_path / "records.f32"
    rec.tofile(path)
    p = subprocess.run([_build(), "gpu", str(path)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
