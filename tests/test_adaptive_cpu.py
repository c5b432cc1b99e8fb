"""Adaptive sampling without a GPU: the three entry points reject a NULL context, and the Python wrappers
(HipRenderer.adaptive_select, render_passes_list, render_adaptive, AdaptiveRender) validate their
arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from pysicalbasedraytracer_amd import AdaptiveRender, HipRenderer, capi, scenes


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


def table_desc():
    table = np.zeros(16 * 8 * 2 * 8, dtype=np.float32)
    rd = desc(spp=2)
    rd.sampler = capi.SAMPLER_TABLE
    rd.sample_table = capi.fptr(table)
    rd.table_dims = 8
    return rd, table


def test_null_context_is_rejected():
    lib = capi.load_library()
    acc = (C.c_float * 6)()
    lst = (C.c_int32 * 1)()
    n = C.c_int(7)
    assert lib.pbr_hip_adaptive_select(None, 1, 2, 0.05, 1e-3, acc, None, 0, lst, C.byref(n), None) == capi.PBR_E_INVALID
    assert n.value == 7
    rd = desc()
    assert lib.pbr_hip_render_passes_list(None, C.byref(rd), 0, 1, lst, 1, acc, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_render_passes_list(None, None, 0, 1, None, 0, acc, None, None) == capi.PBR_E_INVALID
    a = capi.Adaptive(2, 2, 0.05, 1e-3)
    res = capi.AdaptiveResult()
    assert lib.pbr_hip_render_adaptive(None, C.byref(rd), C.byref(a), acc, lst, None, None, C.byref(res)) == capi.PBR_E_INVALID


def test_the_structs_match_the_header():
    assert C.sizeof(capi.Adaptive) == 16 and C.sizeof(capi.AdaptiveResult) == 24
    assert capi.AdaptiveResult.samples.offset == 8 and capi.AdaptiveResult.active_at_end.offset == 16


@pytest.mark.parametrize("kw, what", [
    (dict(samples_done=1), "samples_done"),
    (dict(n_pixels=0), "n_pixels"),
    (dict(n_pixels=1 << 31), "n_pixels"),
    (dict(tolerance=-0.1), "tolerance"),
    (dict(tolerance=float("nan")), "tolerance"),
    (dict(floor=-1.0), "floor"),
    (dict(floor=float("nan")), "floor"),
    (dict(accum_ptr=0), "accum"),
    (dict(list_out_ptr=None), "list_out"),
    (dict(list_in_ptr=64, n_in=129), "n_in"),
    (dict(list_in_ptr=64, n_in=-1), "n_in"),
])
def test_adaptive_select_validates_before_the_device(kw, what):
    r = renderer_without_device()
    args = dict(n_pixels=128, samples_done=2, tolerance=0.05, floor=1e-3, accum_ptr=64, list_out_ptr=64)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        r.adaptive_select(**args)


@pytest.mark.parametrize("kw, what", [
    (dict(samples=0), "samples"),
    (dict(first_sample=-1), "first_sample"),
    (dict(n_list=-1), "n_list"),
    (dict(n_list=129), "n_list"),
    (dict(list_ptr=None), "list is required"),
    (dict(accum_ptr=0), "accum"),
    (dict(first_sample=6, samples=3), "budget"),
])
def test_render_passes_list_validates_before_the_device(kw, what):
    r = renderer_without_device()
    rd = desc(spp=8)
    before = bytes(rd)
    args = dict(first_sample=2, samples=3, list_ptr=64, n_list=5, accum_ptr=64)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        r.render_passes_list(rd, **args)
    assert bytes(rd) == before, "the caller's descriptor was changed"


BAD_ADAPTIVE = [
    (dict(min_samples=1), "min_samples"),
    (dict(min_samples=9), "min_samples"),
    (dict(samples_per_round=0), "samples_per_round"),
    (dict(tolerance=-1e-3), "tolerance"),
    (dict(tolerance=float("nan")), "tolerance"),
    (dict(floor=float("nan")), "floor"),
]


@pytest.mark.parametrize("kw, what", BAD_ADAPTIVE + [(dict(accum_ptr=0), "accum"), (dict(counts_ptr=None), "counts")])
def test_render_adaptive_validates_before_the_device(kw, what):
    r = renderer_without_device()
    rd = desc(spp=8)
    before = bytes(rd)
    args = dict(min_samples=2, samples_per_round=2, tolerance=0.05, floor=1e-3, accum_ptr=64, counts_ptr=64)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        r.render_adaptive(rd, **args)
    assert bytes(rd) == before, "the caller's descriptor was changed"


@pytest.mark.parametrize("kw, what", BAD_ADAPTIVE)
def test_adaptive_render_validates_before_the_device(kw, what):
    args = dict(min_samples=2, samples_per_round=2, tolerance=0.05, floor=1e-3)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        AdaptiveRender(renderer_without_device(), desc(spp=8), **args)


def test_a_sample_table_is_refused():
    r = renderer_without_device()
    rd, _table = table_desc()
    with pytest.raises(ValueError, match="sample table"):
        r.render_passes_list(rd, 0, 1, 64, 4, 64)
    with pytest.raises(ValueError, match="sample table"):
        r.render_adaptive(rd, 2, 1, 0.05, 1e-3, 64, 64)
    with pytest.raises(ValueError, match="sample table"):
        AdaptiveRender(r, rd, min_samples=2)


def test_sobol_budget_is_rounded_up_to_a_power_of_two():
    r = renderer_without_device()
    rd = desc(spp=6, sampler=capi.SAMPLER_SOBOL)
    a = AdaptiveRender(r, rd, min_samples=8, samples_per_round=1)   # 8 <= the rounded budget
    assert a.budget == 8 and a.n_pixels == 16 * 8 and a.samples_done == 0
    with pytest.raises(ValueError, match=r"\[2, 6\]"):
        AdaptiveRender(r, desc(spp=6), min_samples=8)


def test_adaptive_render_restore_checks_shapes():
    a = AdaptiveRender(renderer_without_device(), desc(spp=8), min_samples=2, samples_per_round=2)
    n = 16 * 8
    with pytest.raises(ValueError, match="accumulator of shape"):
        a.restore({"accum": np.zeros((n, 3), np.float32), "counts": np.zeros(n, np.int32)})
    with pytest.raises(ValueError, match="counts of shape"):
        a.restore({"accum": np.zeros((n, 6), np.float32), "counts": np.zeros(n - 1, np.int32)})
    with pytest.raises(ValueError, match="budget"):
        a.restore({"accum": np.zeros((n, 6), np.float32), "counts": np.full(n, 9, np.int32)})
    with pytest.raises(ValueError, match="max_rounds"):
        a.run(max_rounds=0)
    assert a.samples_done == 0
