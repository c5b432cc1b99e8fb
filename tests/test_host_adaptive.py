"""SamplerIntegrator::RenderAdaptive of the C++ host API (include/pbr/pbr.h), in a compiled test
program (tests/cpp_adaptive/adaptive_test.cpp): a huge tolerance leaves RenderSamples(0, minSamples)'s
FrameBuffer, a tolerance of 0 over pixels that all have variance leaves Render's, bit for bit."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pysicalbasedraytracer_amd", "host")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp_adaptive")], check=True)
    return os.path.join(HERE, "cpp_adaptive", "adaptive_test")


def _run(mode, timeout):
    p = subprocess.run([_build(), mode], capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr


def test_render_adaptive_cpu():
    """Bad parameters and a custom sampler are refused before any device call; without a device the
    call fails loudly (no CPU fallback)."""
    if os.path.exists("/dev/kfd") and os.environ.get("PBR_EXPECT_NO_GPU") is None:
        pytest.skip("a GPU is present: the no-device check does not apply")
    _run("cpu", 120)


@pytest.mark.gpu
def test_render_adaptive_gpu():
    """RenderAdaptive against RenderSamples (huge tolerance) and Render (tolerance 0), Whitted and Path."""
    _run("gpu", 300)
