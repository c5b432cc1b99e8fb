"""Progressive rendering without a GPU: pbr_hip_render_passes rejects a NULL context, and the Python
wrappers (HipRenderer.render_passes, ProgressiveRender) validate their arguments before they touch
a device."""
import ctypes as C

import numpy as np
import pytest

from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, capi, scenes


class NoDevice:
    """Stands in for the loaded library: any call through it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")


def renderer_without_device():
    r = HipRenderer.__new__(HipRenderer)
    r.lib = NoDevice()
    r.ctx = C.c_void_p()
    return r


def desc(spp=8, sampler=capi.SAMPLER_HALTON, **kw):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, spp, 3, 1.0, capi.LIGHTS_UNIFORM, sampler, **kw)


def test_null_context_is_rejected():
    lib = capi.load_library()
    acc = (C.c_float * 6)()
    assert lib.pbr_hip_render_passes(None, None, 0, 1, 1, acc, None, None) == capi.PBR_E_INVALID
    rd = desc()
    assert lib.pbr_hip_render_passes(None, C.byref(rd), 0, 1, 1, acc, None, None) == capi.PBR_E_INVALID


@pytest.mark.parametrize("kw, what", [
    (dict(first_sample=0, samples_per_pass=0, accum_ptr=64, n_passes=1), "samples_per_pass"),
    (dict(first_sample=-1, samples_per_pass=1, accum_ptr=64, n_passes=1), "first_sample"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=64, n_passes=0), "no passes"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=64), "no passes"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=None, n_passes=1), "accum"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=0, n_passes=1), "accum"),
    (dict(first_sample=0, samples_per_pass=3, accum_ptr=64, n_passes=3), "budget"),
    (dict(first_sample=6, samples_per_pass=3, accum_ptr=64, n_passes=1), "budget"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=64, rgb_ptrs=[64, 64], rgba_ptrs=[64]), "outputs"),
    (dict(first_sample=0, samples_per_pass=1, accum_ptr=64, rgb_ptrs=[64, 64], n_passes=3), "rgb_ptrs"),
])
def test_render_passes_validates_before_the_device(kw, what):
    r = renderer_without_device()
    rd = desc(spp=8)
    before = bytes(rd)
    with pytest.raises(ValueError, match=what):
        r.render_passes(rd, **kw)
    assert bytes(rd) == before, "the caller's descriptor was changed"


def test_render_passes_refuses_a_sample_table():
    r = renderer_without_device()
    table = np.zeros(16 * 8 * 2 * 8, dtype=np.float32)
    rd = desc(spp=2, sampler=capi.SAMPLER_HALTON)
    rd.sampler = capi.SAMPLER_TABLE
    rd.sample_table = capi.fptr(table)
    rd.table_dims = 8
    with pytest.raises(ValueError, match="sample table"):
        r.render_passes(rd, 0, 1, 64, n_passes=1)
    with pytest.raises(ValueError, match="sample table"):
        ProgressiveRender(r, rd)


def test_sobol_budget_is_rounded_up_to_a_power_of_two():
    rd = desc(spp=6, sampler=capi.SAMPLER_SOBOL)
    assert HipRenderer.sample_budget(rd) == 8
    assert HipRenderer.sample_budget(desc(spp=6)) == 6
    r = renderer_without_device()
    with pytest.raises(ValueError, match="budget of 8"):
        r.render_passes(rd, 0, 3, 64, n_passes=3)


def test_progressive_render_validates_before_the_device():
    r = renderer_without_device()
    rd = desc(spp=8)
    p = ProgressiveRender(r, rd)
    assert p.samples_done == 0 and p.budget == 8 and p.n_pixels == 16 * 8
    for n, passes in [(0, 1), (1, 0), (-2, 1), (9, 1), (3, 3)]:
        with pytest.raises(ValueError):
            p.step(n, passes)
    with pytest.raises(ValueError, match="at least 2"):
        p.variance()
    assert p.samples_done == 0
    with pytest.raises(ValueError, match="shape"):
        p.restore({"samples_done": 2, "accum": np.zeros((5, 6), np.float32)})
    with pytest.raises(ValueError, match="budget"):
        p.restore({"samples_done": 9, "accum": np.zeros((16 * 8, 6), np.float32)})
    rd0 = desc(spp=8)
    rd0.spp = 0
    with pytest.raises(ValueError):
        ProgressiveRender(r, rd0)
