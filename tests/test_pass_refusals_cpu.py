"""The three Python wrappers that take a window of samples (HipRenderer.render_passes, render_aov,
render_passes_list) refuse the same bad windows in the same words, before any library call, and leave
the caller's descriptor as it was.  No GPU: the library is a stand-in that fails the test when called."""
import ctypes as C
import re

import numpy as np
import pytest

from pysicalbasedraytracer_amd import HipRenderer, capi, scenes


class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")


def renderer_without_device():
    r = HipRenderer.__new__(HipRenderer)
    r.lib = NoDevice()
    r.ctx = C.c_void_p()
    return r


def desc(spp=8, sampler=capi.SAMPLER_HALTON):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, spp, 3, 1.0, capi.LIGHTS_UNIFORM, sampler)


_table = np.zeros(16 * 8 * 8 * 8, dtype=np.float32)


def table_desc():
    rd = desc()
    rd.sampler, rd.sample_table, rd.table_dims = capi.SAMPLER_TABLE, capi.fptr(_table), 8
    return rd


# wrapper -> (what it calls its sample count, the accumulator's floats per pixel, the call)
WRAPPERS = {
    "render_passes": ("samples_per_pass", 6,
                      lambda r, rd, first, samples, accum: r.render_passes(rd, first, samples, accum, n_passes=1)),
    "render_aov": ("samples", 8, lambda r, rd, first, samples, accum: r.render_aov(rd, first, samples, accum)),
    "render_passes_list": ("samples", 6,
                           lambda r, rd, first, samples, accum: r.render_passes_list(rd, first, samples, 64, 5, accum)),
}
# case -> (descriptor, first_sample, samples, accum, the message after "<wrapper>: ")
BAD = {
    "samples_0": (desc, 0, 0, 64, "{samples} must be >= 1"),
    "first_sample_-1": (desc, -1, 1, 64, "first_sample must be >= 0"),
    "accum_None": (desc, 0, 1, None, "accum is required (a device buffer of {floats} float32 per pixel)"),
    "accum_0": (desc, 0, 1, 0, "accum is required (a device buffer of {floats} float32 per pixel)"),
    "table": (table_desc, 0, 1, 64, "no passes over a sample table"),
    "halton_one_past": (desc, 6, 3, 64, "samples [6, 9) run past the budget of 8 samples per pixel"),
    "sobol_6_one_past": (lambda: desc(6, capi.SAMPLER_SOBOL), 6, 3, 64, "samples [6, 9) run past the budget of 8 samples per pixel"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_a_bad_window_is_refused_before_the_device(wrapper, case):
    samples_arg, floats, call = WRAPPERS[wrapper]
    make, first, samples, accum, text = BAD[case]
    rd = make()
    before = bytes(rd)
    message = f"{wrapper}: " + text.format(samples=samples_arg, floats=floats)
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        call(renderer_without_device(), rd, first, samples, accum)
    assert bytes(rd) == before, "the caller's descriptor was changed"


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_the_last_window_of_the_budget_is_not_refused(wrapper):
    """[5, 8) of a Sobol budget of 8 (spp 6) passes the checks: the stand-in library is reached."""
    with pytest.raises(AssertionError, match="was called"):
        WRAPPERS[wrapper][2](renderer_without_device(), desc(6, capi.SAMPLER_SOBOL), 5, 3, 64)
