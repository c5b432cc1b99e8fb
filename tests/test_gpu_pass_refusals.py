"""The four entry points that render a window of a frame's samples — pbr_hip_render_passes,
pbr_hip_render_passes_list, pbr_hip_render_adaptive and pbr_hip_render_aov — called straight through the
C-ABI with exactly one bad argument: the code, the message (it names the entry point and, for a window
past the budget, the budget), and that the refusal leaves no state behind: a valid call on the same
context afterwards gives the bits of the same call on a fresh context.  A 16x8 frame at spp 8."""
import ctypes as C

import numpy as np
import pytest
import torch

from pysicalbasedraytracer_amd import HipRenderer, capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
W, H, SPP = 16, 8, 8
NPX = W * H
ENTRIES = ("render_passes", "render_passes_list", "render_adaptive", "render_aov")
BATCH_RULE = "device outputs, no stats, no sample table, n >= 1"   # render_passes words it as render_frames does


def desc(spp=SPP, sampler=capi.SAMPLER_HALTON, on_device=1, stats=0, table=None):
    _, rd = scenes.config_c1(W, H, spp)
    d = scenes.render_desc(rd.camera, rd.integrator, spp, rd.max_depth, rd.rr_threshold, rd.light_strategy, sampler,
                           sample_table=table)
    d.outputs_on_device, d.collect_stats = on_device, stats
    return d


def buffers(entry):
    """Device buffers of one call: the accumulator first; filled so that an unwritten entry shows."""
    t = {"accum": torch.zeros((NPX, 8 if entry == "render_aov" else 6), dtype=torch.float32, device=DEV)}
    if entry == "render_aov":
        t["out"] = torch.full((NPX, 8), -1.0, dtype=torch.float32, device=DEV)
    else:
        t["rgb"] = torch.full((NPX, 3), -1.0, dtype=torch.float32, device=DEV)
        t["rgba"] = torch.full((NPX, 4), 7, dtype=torch.uint8, device=DEV)
    if entry == "render_adaptive":
        t["counts"] = torch.full((NPX,), -1, dtype=torch.int32, device=DEV)
    if entry == "render_passes_list":
        t["list"] = torch.arange(1, NPX, 3, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    return t


def call(hip, entry, t, d, first=0, samples=2, accum=True, min_samples=2, per_round=2):
    """One call of `entry` on the buffers t; accum=False passes NULL."""
    lib, acc = hip.lib, t["accum"].data_ptr() if accum else None
    if entry == "render_passes":
        rgb, rgba = (C.c_void_p * 1)(t["rgb"].data_ptr()), (C.c_void_p * 1)(t["rgba"].data_ptr())
        return lib.pbr_hip_render_passes(hip.ctx, C.byref(d), first, samples, 1, acc, rgb, rgba)
    if entry == "render_passes_list":
        return lib.pbr_hip_render_passes_list(hip.ctx, C.byref(d), first, samples, t["list"].data_ptr(), t["list"].numel(), acc,
                                              t["rgb"].data_ptr(), t["rgba"].data_ptr())
    if entry == "render_aov":
        return lib.pbr_hip_render_aov(hip.ctx, C.byref(d), first, samples, acc, t["out"].data_ptr())
    a, res = capi.Adaptive(min_samples, per_round, 0.05, 1e-3), capi.AdaptiveResult()
    return lib.pbr_hip_render_adaptive(hip.ctx, C.byref(d), C.byref(a), acc, t["counts"].data_ptr(), t["rgb"].data_ptr(),
                                       t["rgba"].data_ptr(), C.byref(res))


def valid(hip, entry):
    """A valid call of `entry`, waited for: its buffers as host arrays."""
    t = buffers(entry)
    rc = call(hip, entry, t, desc())
    assert rc == capi.PBR_OK, hip.lib.pbr_hip_last_error(hip.ctx).decode()
    hip.sync()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    r.upload(scenes.config_c1(W, H, SPP)[0])
    yield r
    r.close()


@pytest.fixture(scope="module")
def fresh():
    """Each entry point's valid call on a context that has seen nothing else, computed once."""
    out = {}
    for entry in ENTRIES:
        r = HipRenderer(0)
        r.upload(scenes.config_c1(W, H, SPP)[0])
        out[entry] = valid(r, entry)
        r.close()
    return out


_table = np.zeros((H, W, SPP, 8), dtype=np.float32)
PAST = "samples [6, 9) run past the budget of 8 samples per pixel"
# case -> (descriptor, call arguments, code, message after "<entry>: " — per entry where the words differ)
CASES = {
    "samples_0": (desc, dict(samples=0, per_round=0), capi.PBR_E_INVALID,
                  {"render_passes": "samples_per_pass must be >= 1", "render_adaptive": "samples_per_round must be >= 1",
                   None: "samples must be >= 1"}),
    "first_sample_-1": (desc, dict(first=-1), capi.PBR_E_INVALID, {None: "first_sample must be >= 0"}),
    "accum_null": (desc, dict(accum=False), capi.PBR_E_INVALID,
                   {"render_aov": "accum must be a device buffer of 8 floats per pixel",
                    "render_adaptive": "parameters, accum and counts are required",
                    None: "accum must be a device buffer of 6 floats per pixel"}),
    "host_outputs": (lambda: desc(on_device=0), {}, capi.PBR_E_INVALID,
                     {"render_passes": BATCH_RULE, None: "device outputs, no stats"}),
    "collect_stats": (lambda: desc(stats=1), {}, capi.PBR_E_INVALID,
                      {"render_passes": BATCH_RULE, None: "device outputs, no stats"}),
    "table": (lambda: desc(sampler=capi.SAMPLER_TABLE, table=_table), {}, capi.PBR_E_UNSUPPORTED,
              {None: "no passes over a sample table"}),
    "halton_one_past": (desc, dict(first=6, samples=3, min_samples=9), capi.PBR_E_INVALID,
                        {"render_adaptive": "min_samples must be in [2, 8] (the budget)", None: PAST}),
    "sobol_6_one_past": (lambda: desc(spp=6, sampler=capi.SAMPLER_SOBOL), dict(first=6, samples=3, min_samples=9),
                         capi.PBR_E_INVALID, {"render_adaptive": "min_samples must be in [2, 8] (the budget)", None: PAST}),
}
# (pbr_hip_render_adaptive has no first_sample)
PARAMS = [(e, c) for e in ENTRIES for c in sorted(CASES) if (e, c) != ("render_adaptive", "first_sample_-1")]


@pytest.mark.parametrize("entry,case", PARAMS, ids=lambda v: v)
def test_one_bad_argument_is_refused_and_leaves_no_state(hip, fresh, entry, case):
    make, kw, code, texts = CASES[case]
    t = buffers(entry)
    before = {k: v.cpu().numpy() for k, v in t.items()}
    rc = call(hip, entry, t, make(), **kw)
    message = hip.lib.pbr_hip_last_error(hip.ctx).decode()
    print(f"{entry} {case}: {rc} {message!r}")
    assert rc == code
    assert message == f"{entry}: " + texts.get(entry, texts[None])
    hip.sync()
    torch.cuda.synchronize()
    assert same_bits(before, {k: v.cpu().numpy() for k, v in t.items()}), "a refused call wrote to its buffers"
    assert same_bits(fresh[entry], valid(hip, entry)), "a valid call after the refusal differs from a fresh context's"
