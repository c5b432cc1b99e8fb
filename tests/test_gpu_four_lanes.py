"""The four-lane, own-queue topology between calls, and the memory the lanes take.

With four lanes and a caller's stream, lane 0 runs on the context's stream (pbr_kernels.hip wf_fork):
which stream is lane 0 is state of the call, and the join and the per-frame events (pbr_hip_wait_frame)
go through it.  test_gpu_batch.py, test_gpu_progressive.py and test_gpu_parity.py run that topology one
call at a time; here calls of different topologies follow each other on one context and one stream,
and a second stream takes frames out of the middle.  Everything is compared on the bits with the
megakernel and the oracle, on the small Path scene of test_gpu_progressive.py (and its oracle cache).

test_lane_bytes_within_estimate holds the plan's bytes_per_sample — which lane_budget relies on to
keep the lanes under 3/4 of the free device memory — to be an upper bound of what the lanes allocate."""
import numpy as np
import pytest
import torch

import test_gpu_progressive as TP
from lane_schedules import MORE, ROTATING, assert_regime
from pysicalbasedraytracer_amd import HipRenderer, capi, scenes

pytestmark = pytest.mark.gpu

DEV = TP.DEV
bits = TP.bits


@pytest.fixture()
def hip():
    r = HipRenderer(0)   # a context of its own per test: its lane buffers are what the test made them
    yield r
    r.close()


def outputs(npx, n):
    return ([torch.full((npx, 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(n)],
            [torch.zeros((npx, 4), dtype=torch.uint8, device=DEV) for _ in range(n)])


def ptrs(ts):
    return [t.data_ptr() for t in ts]


def test_four_lane_calls_interleave(hip):
    """On one context and one caller's stream: a 4-lane frame (6 chunks), a 3-lane frame, a 4-lane
    batch of 3 frames (6 chunks each, forked and joined per frame), frames of that batch copied out on a
    second stream after pbr_hip_wait_frame, 4-lane passes of 2 samples (2 chunks: they rotate over the
    lanes) — then a megakernel batch on the same stream, whose frame events must not go to the stream
    the 4-lane calls made lane 0.  Every image is the megakernel's and the oracle's bits.

    Ordering (include/pbr_hip.h): calls on one stream follow each other, so nothing waits on the host
    between the calls of one schedule.  pbr_hip_set_schedule itself waits for the context's queued
    work — the setting holds for later renders only — so the changes to three lanes and back, and to the
    megakernel, are host waits the interface imposes.  The output buffers are filled on torch's stream,
    which the library's streams do not wait for: ordering those fills before the renders is the caller's
    duty, done here by one device synchronisation before the first call."""
    s, rd = TP.scene("path")
    npx = HipRenderer.n_pixels(rd)
    c, c8 = TP.oracle("path", s, rd, rd.spp)
    hip.upload(s)
    hip.set_schedule(kernels=capi.KERNELS_MEGAKERNEL)
    mk, mk8, _ = hip.render(rd)
    assert np.array_equal(bits(mk), bits(c)) and np.array_equal(mk8, c8)

    st, other = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    four = dict(chunk_log2=13, lanes=4)
    (f4, f3), (f4_8, f3_8) = outputs(npx, 2)
    brgb, brgba = outputs(npx, 3)
    prgb, prgba = outputs(npx, 4)
    mrgb, mrgba = outputs(npx, 3)
    acc = TP.new_accum(rd)
    torch.cuda.synchronize()   # the fills above (see the docstring)

    hip.set_schedule(**four)
    hip.render_device(rd, f4.data_ptr(), f4_8.data_ptr(), stream=st.cuda_stream, sync=False)
    assert_regime(hip.last_chunks(), MORE, caller_stream=True, batch=False)
    hip.set_schedule(chunk_log2=13, lanes=3)
    hip.render_device(rd, f3.data_ptr(), f3_8.data_ptr(), stream=st.cuda_stream, sync=False)
    plan = hip.last_chunks()
    assert plan["lanes"] == 3 and plan["n_chunks"] > 3 and not plan["lane0_on_ctx_stream"], plan
    hip.set_schedule(**four)
    hip.render_frames(rd, ptrs(brgb), ptrs(brgba), stream=st.cuda_stream)
    assert_regime(hip.last_chunks(), MORE, caller_stream=True, batch=True)
    copies = []
    for f in (1, 0, 2):   # each copy on `other` runs after its frame, whatever else is queued
        hip.wait_frame(other.cuda_stream, f)
        with torch.cuda.stream(other):
            copies.append((f, brgb[f].clone(), brgba[f].clone()))
    hip.render_passes(rd, 0, 2, acc.data_ptr(), ptrs(prgb), ptrs(prgba), stream=st.cuda_stream)
    assert_regime(hip.last_chunks(), ROTATING, caller_stream=True, batch=True)
    pass_copies = []
    for p in (3, 1):
        hip.wait_frame(other.cuda_stream, p)
        with torch.cuda.stream(other):
            pass_copies.append((p, prgb[p].clone(), prgba[p].clone()))
    hip.set_schedule(kernels=capi.KERNELS_MEGAKERNEL)
    hip.render_frames(rd, ptrs(mrgb), ptrs(mrgba), stream=st.cuda_stream)
    plan = hip.last_chunks()
    assert plan["lanes"] == 0 and plan["n_chunks"] == 0 and not plan["lane0_on_ctx_stream"], plan
    hip.wait_frame(other.cuda_stream, 2)
    with torch.cuda.stream(other):
        mega_copy = (mrgb[2].clone(), mrgba[2].clone())
    other.synchronize()
    hip.sync()
    torch.cuda.synchronize()

    def same(what, rgb, rgba, want=mk, want8=mk8):
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(want)), what
        assert np.array_equal(rgba.cpu().numpy(), want8), what

    same("4-lane frame", f4, f4_8)
    same("3-lane frame", f3, f3_8)
    for f in range(3):
        same(f"4-lane batch, frame {f}", brgb[f], brgba[f])
        same(f"megakernel batch, frame {f}", mrgb[f], mrgba[f])
    for f, rgb, rgba in copies:
        same(f"4-lane batch, frame {f} copied on a second stream after wait_frame", rgb, rgba)
    same("megakernel batch, frame 2 copied on a second stream after wait_frame", *mega_copy)
    for p in range(4):
        TP.check("path", s, rd, 2 * (p + 1), prgb[p], prgba[p], f"4-lane rotating passes, pass {p}")
    for p, rgb, rgba in pass_copies:
        TP.check("path", s, rd, 2 * (p + 1), rgb, rgba, f"pass {p} copied on a second stream after wait_frame")
    same("the last pass", prgb[3], prgba[3])


def five_lights():
    s, rd = scenes.config_c2_lights(256, 256, 64, mesh=TP.small_dragon(40))   # the sky and two point lights
    s.point_light((0.5, 1.5, -2.0), (2.0, 4.0, 3.0))
    s.point_light((-2.0, 2.5, 0.5), (5.0, 2.0, 2.0))
    return s, rd


LANE_BYTE_SCENES = {
    "whitted_sky": lambda: scenes.config_c2(256, 256, 64, mesh=TP.small_dragon(48), sky=scenes.procedural_sky(128, 64)),
    "whitted_5_lights": five_lights,
    "path": lambda: scenes.config_c4(256, 256, 64, mesh=TP.small_dragon(40)),
    "volpath": lambda: scenes.config_c5(256, 256, 64, mesh=TP.small_dragon(40)),
}


@pytest.mark.parametrize("kind", sorted(LANE_BYTE_SCENES))
def test_lane_bytes_within_estimate(hip, kind):
    """Four lanes of 2^20-sample chunks over a 256x256 frame at 64 spp (2^22 samples, four chunks): the
    bytes the context's lanes hold afterwards stay within lanes x bytes_per_sample x qcap, the estimate
    lane_budget's plans are sized by.  (Measured ratios: profiles/lane_bytes.md.)"""
    s, rd = LANE_BYTE_SCENES[kind]()
    if kind == "whitted_sky":
        assert len(s.lights) == 1 and s.lights[0].type == capi.LIGHT_SKYBOX
    if kind == "whitted_5_lights":
        assert len(s.lights) == 5
    hip.upload(s)
    assert hip.last_chunks()["held_lane_bytes"] == 0
    hip.set_schedule(chunk_log2=20, lanes=4)
    rgb, _, _ = hip.render(rd, rgba=False)
    assert np.isfinite(rgb).all()
    plan = hip.last_chunks()
    assert (plan["lanes"], plan["chunk_log2"], plan["n_chunks"]) == (4, 20, 4) and plan["cap"] == 2 ** 20, plan
    estimate = plan["lanes"] * plan["bytes_per_sample"] * plan["qcap"]
    held = plan["held_lane_bytes"]
    print(f"{kind}: lanes hold {held} B, estimate {estimate:.0f} B ({plan['bytes_per_sample']:.0f} B per sample), "
          f"ratio {held / estimate:.4f}")
    assert 0 < held <= estimate, f"{kind}: the lanes hold {held} B, over the estimate of {estimate:.0f} B"
