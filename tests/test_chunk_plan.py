"""The chunk plan the renders run (pysicalbasedraytracer_amd/csrc/pbr_chunk_plan.h), asked through
pbr_hip_plan_chunks: a pure function, so no GPU is needed.

The sweep crosses the three integrators with frame sizes around the one-pixel, one-block, one-chunk
and full-size cases, sample counts, depths and light counts (which set Whitted's bytes per sample and
its record bound), single frames and batches, and lane budgets from "unknown" (0) through 1e8 to 3e11
bytes in half decades — under the default request and under every chunk_log2, lanes and serial value
pbr_hip_set_schedule accepts.  Depth and lights reach the plan only through bytes_per_sample and
Whitted's default chunk, so the explicit requests are crossed with their extremes ((0, 0) and (50, 5))
and the default request with all of them.  Every point is held to the invariants the render loops
rely on; the documented plans of the benchmark configs are pinned at an idle MI355X's budget
(ref_scenes.NOMINAL_LANE_BUDGET)."""
import ctypes as C
import itertools
import math

import pytest

import ref_scenes as RS
from pysicalbasedraytracer_amd import capi, scenes

INTEGRATORS = (capi.INTEGRATOR_WHITTED, capi.INTEGRATOR_PATH, capi.INTEGRATOR_VOLPATH)
N_PIXELS = (1, 2, 255, 256, 257, 5184, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 1920 * 1080, 3840 * 2160)
SPP = (1, 3, 64, 256, 1024)
MAX_DEPTH = (0, 1, 5, 50)
LIGHTS = (0, 1, 5)
BUDGETS = (0.0,) + tuple(10.0 ** (8 + k / 2) for k in range(8))   # 0, 1e8, 3.16e8, ..., 3.16e11
assert BUDGETS[1] == 1e8 and 3e11 < BUDGETS[-1] < 3.2e11
CHUNK_LOG2 = (0,) + tuple(range(10, 29))
LANES = (0, 1, 2, 3, 4)
WF_BLOCKS = capi.WALK_SEGMENTS   # segments of a queue = workgroups of the queue kernels (pbr_hip.h)
BATCH_LANE_BYTES = 48e9          # a batch's one-chunk frames with the budget unknown (pbr_chunk_plan.h kBatchLaneBytes)
MIN_LOG2, PATH_MAX_LOG2, WHITTED_MAX_LOG2 = 20, 27, 25


class Planner:
    """pbr_hip_plan_chunks with the structures reused (a few hundred thousand calls)."""

    def __init__(self):
        self.fn = capi.load_library().pbr_hip_plan_chunks
        self.q, self.s, self.out = capi.ChunkQuery(), capi.Schedule(), capi.ChunkPlan()
        self.q.scene_fusable = 1
        self.args = (C.byref(self.s), C.byref(self.q), C.byref(self.out))

    def __call__(self, integ, npx, spp, depth, lights, batch, budget, log2=0, lanes=0, serial=0, sky=0):
        q, s = self.q, self.s
        q.integrator, q.n_pixels, q.spp, q.max_depth, q.n_lights, q.sky_light = integ, npx, spp, depth, lights, sky
        q.batch, q.lane_budget = batch, budget
        s.chunk_log2, s.lanes, s.serial = log2, lanes, serial
        assert self.fn(*self.args) == capi.PBR_OK
        return self.out


def check_point(p, integ, npx, spp, batch, budget, log2, lanes, serial):
    """The invariants of one plan; returns (lanes, chunk_log2, whether a single frame collapsed to one
    chunk on one lane) for the monotonicity check."""
    where = (integ, npx, spp, batch, budget, log2, lanes, serial)
    n, cp = p.n_chunks, p.chunk_pixels
    assert n >= 1 and cp >= 1, where
    assert n * cp >= npx > (n - 1) * cp, where
    assert p.cap == cp * spp, where
    assert p.seg_cap > 0 and p.seg_cap % 256 == 0, where
    assert p.qcap >= p.cap and p.qcap >= p.seg_cap * WF_BLOCKS, where
    assert 1 <= p.lanes <= 4, where
    if serial:
        assert p.lanes == 1, where
    if lanes and not serial:
        assert p.lanes <= lanes, where
    max_log2 = WHITTED_MAX_LOG2 if integ == capi.INTEGRATOR_WHITTED else PATH_MAX_LOG2
    assert 10 <= p.chunk_log2 <= max_log2, where
    if log2:
        assert p.chunk_log2 == min(log2, max_log2), where
    elif budget > 0:   # the default chunk fits the budget, down to the 2^20 floor
        assert p.chunk_log2 >= MIN_LOG2, where
        assert p.lanes * p.bytes_per_sample * 2.0 ** p.chunk_log2 <= budget or p.chunk_log2 == MIN_LOG2, where
    pow2 = max(1, 2 ** p.chunk_log2 // spp)   # the power-of-two chunk (one pixel at the least)
    n_pow2 = -(-npx // pow2)
    if n_pow2 >= 24:   # balanced: equal chunks (which may pass 2^chunk_log2 samples), a whole number per lane
        assert n % p.lanes == 0 and p.lanes <= n <= n_pow2, where
    else:
        assert cp == (npx if n == 1 else pow2) and n == n_pow2, where
    if n >= 24:
        assert n % p.lanes == 0, where
    assert p.bytes_per_sample > 0 and p.lane_budget == budget, where
    # the lanes before a one-chunk frame gives some up: the request, or the default 3 (Path: 4 where
    # four lanes of 2^27-sample chunks fit a known budget and the chunk is left to the library)
    want = 1 if serial else lanes or 3
    if (not serial and not lanes and not log2 and integ == capi.INTEGRATOR_PATH and budget > 0 and
            4 * p.bytes_per_sample * 2.0 ** PATH_MAX_LOG2 <= budget):
        want = 4
    if n == 1:
        if batch:
            per_lane = p.bytes_per_sample * npx * spp
            fit = math.floor((budget if budget > 0 else BATCH_LANE_BYTES) / per_lane)
            assert p.lanes == max(1, min(want, fit)), where
        else:
            assert p.lanes == 1, where
    else:
        assert p.lanes == want, where
    return p.lanes, p.chunk_log2, n == 1 and not batch


def sweep_budgets(plan, integ, npx, spp, depth, lights, batch, log2, lanes, serial):
    prev_lanes = prev_log2 = 0
    for budget in BUDGETS:
        got = check_point(plan(integ, npx, spp, depth, lights, batch, budget, log2, lanes, serial),
                          integ, npx, spp, batch, budget, log2, lanes, serial)
        # A larger known budget never costs chunk size or lanes (0 = unknown stands apart).  One
        # exception is the design's own: a single frame that a larger chunk holds whole runs on one lane
        # (splitting it only adds launch tails, pbr_chunk_plan.h), so there the lanes are not compared.
        if budget == 0:
            continue
        where = (integ, npx, spp, depth, lights, batch, budget, log2, lanes, serial)
        got_lanes, got_log2, collapsed = got
        assert got_log2 >= prev_log2, where
        prev_log2 = got_log2
        if not collapsed:
            assert got_lanes >= prev_lanes, where
            prev_lanes = got_lanes


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_default_request_over_the_whole_sweep(integ):
    plan = Planner()
    for npx, spp, depth, lights, batch in itertools.product(N_PIXELS, SPP, MAX_DEPTH, LIGHTS, (0, 1)):
        sweep_budgets(plan, integ, npx, spp, depth, lights, batch, 0, 0, 0)


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_every_schedule_request(integ):
    plan = Planner()
    for (depth, lights), npx, spp, batch in itertools.product(((0, 0), (50, 5)), N_PIXELS, SPP, (0, 1)):
        for log2, lanes, serial in itertools.product(CHUNK_LOG2, LANES, (0, 1)):
            sweep_budgets(plan, integ, npx, spp, depth, lights, batch, log2, lanes, serial)


def test_unknown_budget_is_a_fixed_default():
    """The memory query failed: Path / VolPath plan 2^26-sample chunks on 3 lanes (not an unbounded
    2^27), Whitted its record-bounded default."""
    plan = Planner()
    for integ in (capi.INTEGRATOR_PATH, capi.INTEGRATOR_VOLPATH):
        p = plan(integ, 3840 * 2160, 1024, 8, 1, 1, 0.0)
        assert (p.lanes, p.chunk_log2) == (3, 26)
    p = plan(capi.INTEGRATOR_WHITTED, 1920 * 1080, 64, 5, 1, 1, 0.0, sky=1)
    assert (p.lanes, p.chunk_log2, p.n_chunks) == (3, 25, 4)


def test_bytes_per_sample_follows_the_scene():
    """Whitted's estimate grows with depth and lights and with a deferred SkyBox; Path's and VolPath's
    are constants (VolPath's the larger)."""
    plan = Planner()
    w = lambda depth, lights, sky=0: plan(capi.INTEGRATOR_WHITTED, 5184, 64, depth, lights, 0, 1e11, sky=sky).bytes_per_sample
    assert w(5, 1) < w(6, 1) < w(6, 5) and w(5, 1) < w(5, 1, sky=1) and w(0, 1) == w(1, 1)
    assert w(5, 5, sky=1) == w(5, 5)   # (several lights: none is deferred)
    p = [plan(i, 5184, 64, d, l, 0, 1e11).bytes_per_sample for i in INTEGRATORS[1:] for d, l in ((1, 0), (50, 5))]
    assert p[0] == p[1] < p[2] == p[3]


def test_invalid_queries_are_rejected():
    lib = capi.load_library()
    out = capi.ChunkPlan()
    ok = dict(integrator=capi.INTEGRATOR_PATH, n_pixels=100, spp=4, max_depth=5, n_lights=1, lane_budget=1e9)
    assert lib.pbr_hip_plan_chunks(None, C.byref(capi.ChunkQuery(**ok)), C.byref(out)) == capi.PBR_OK
    assert lib.pbr_hip_plan_chunks(None, None, C.byref(out)) == capi.PBR_E_INVALID
    assert lib.pbr_hip_plan_chunks(None, C.byref(capi.ChunkQuery(**ok)), None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_last_chunks(None, C.byref(out)) == capi.PBR_E_INVALID
    for bad in (dict(integrator=3), dict(integrator=-1), dict(n_pixels=0), dict(spp=0), dict(n_lights=-1),
                dict(lane_budget=-1.0), dict(lane_budget=float("nan"))):
        assert lib.pbr_hip_plan_chunks(None, C.byref(capi.ChunkQuery(**{**ok, **bad})), C.byref(out)) == capi.PBR_E_INVALID, bad
    for bad in (dict(chunk_log2=9), dict(chunk_log2=29), dict(lanes=5), dict(lanes=-1), dict(serial=2), dict(kernels=2),
                dict(fuse_camera=3)):
        assert lib.pbr_hip_plan_chunks(C.byref(capi.Schedule(**bad)), C.byref(capi.ChunkQuery(**ok)),
                                       C.byref(out)) == capi.PBR_E_INVALID, bad


def test_fused_camera_rule():
    """Whitted fuses the camera into the level-0 shade in frames of at least max(2, lanes) chunks, in
    a batch's rotating frames, or on request — never with several lights, a scene that cannot, or
    FUSE_OFF; Path and VolPath never."""
    W = capi.INTEGRATOR_WHITTED
    kw = dict(max_depth=5, n_lights=1, sky_light=True, lane_budget=RS.NOMINAL_LANE_BUDGET)
    big, small = 1920 * 1080, 5184
    assert capi.plan_chunks(W, big, 64, **kw)["fused_camera"]
    assert not capi.plan_chunks(W, small, 64, **kw)["fused_camera"]                 # one chunk, single frame
    assert capi.plan_chunks(W, small, 64, batch=True, **kw)["fused_camera"]         # rotating
    assert capi.plan_chunks(W, small, 64, schedule=capi.Schedule(fuse_camera=capi.FUSE_ON), **kw)["fused_camera"]
    assert not capi.plan_chunks(W, big, 64, schedule=capi.Schedule(fuse_camera=capi.FUSE_OFF), **kw)["fused_camera"]
    assert not capi.plan_chunks(W, big, 64, scene_fusable=False, **kw)["fused_camera"]
    assert not capi.plan_chunks(W, big, 64, **{**kw, "n_lights": 5, "sky_light": False})["fused_camera"]
    assert not capi.plan_chunks(capi.INTEGRATOR_PATH, big, 64, **kw)["fused_camera"]
    # two chunks on three lanes: fewer than max(2, lanes), so the separate camera kernel
    assert not capi.plan_chunks(W, 2 ** 20, 64, **kw)["fused_camera"]


@pytest.mark.parametrize("config,want", [
    ("C2", dict(n_chunks=4, lanes=3, fused_camera=True, chunk_log2=25)),
    ("C3", dict(lanes=4, chunk_log2=27, n_chunks=4)),
    ("C4", dict(n_chunks=64, chunk_pixels=129600, lanes=4, chunk_log2=27)),
    ("C5", dict(lanes=3, chunk_log2=27, n_chunks=8)),
])
@pytest.mark.parametrize("batch", [False, True])
def test_documented_plans_at_an_idle_devices_budget(config, want, batch):
    """DESIGN.md §4's schedules of the benchmark configs, single frames and bench.py's batches."""
    s, rd = scenes.CONFIGS[config]()
    plan = RS.scene_plan(s, rd, batch=batch)
    assert {k: plan[k] for k in want} == want, plan
