"""Adaptive sampling: pbr_hip_adaptive_select, pbr_hip_render_passes_list, pbr_hip_render_adaptive.

The stopping rule is restated here in numpy float32 from its definition (it has no square root and no
transcendental, so the restatement decides exactly as the device does).  A listed pass is pinned to the
oracle as the uniform passes are: a listed pixel equals the oracle's render at the pixel's sample count.
The counts a whole adaptive render must produce come from code it does not run — accumulator snapshots
of pbr_hip_render_passes (pinned to the oracle's in-order sums by test_gpu_progressive.py), or sums of the
oracle's per-sample radiance — put through the restated rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import test_gpu_progressive as TP   # its scenes, schedules and cache of oracle frames (shared, not recomputed)
from pysicalbasedraytracer_amd import AdaptiveRender, HipRenderer, capi, scenes, tiles_for_rank

pytestmark = pytest.mark.gpu

DEV = TP.DEV
bits = TP.bits
f32 = np.float32


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


# ------------------------------------------------------------------ the rule, restated
def rule(acc, k, tolerance, floor):
    """(active, E) per pixel of acc [n, 6] = Σ L.rgb, Σ L².rgb with k samples done: float32, in this order."""
    acc = np.asarray(acc, dtype=f32)
    S, Q = acc[:, :3], acc[:, 3:]
    with np.errstate(all="ignore"):
        n = f32(k)
        m = S / n
        d = Q - S * m
        v = np.where(d > 0, d, f32(0))                      # (a NaN d gives 0)
        E = ((v[:, 0] + v[:, 1]) + v[:, 2]) / (n * (n - f32(1)))
        M = (m[:, 0] + m[:, 1]) + m[:, 2]
        B = np.where(M > f32(floor), M, f32(floor))
        T = f32(tolerance) * B
        active = E > T * T                                   # (any NaN: not active)
    assert E.dtype == f32 and T.dtype == f32
    return active, E


def expected_counts(snapshots, min_samples, per_round, budget, tolerance, floor):
    """Counts of a whole adaptive render from whole-frame accumulator snapshots {k: acc}: a pixel found
    not active is never reconsidered.  Also the number active after the first select."""
    n = next(iter(snapshots.values())).shape[0]
    counts = np.full(n, min_samples, np.int32)
    alive = np.ones(n, bool)
    k, first_active = min_samples, None
    while True:
        alive &= rule(snapshots[k], k, tolerance, floor)[0]
        if first_active is None:
            first_active = int(alive.sum())
        if not alive.any() or k >= budget:
            return counts, first_active
        k += min(per_round, budget - k)
        counts[alive] = k


# ------------------------------------------------------------------ 1. select against the restatement
SIZES = [1, 63, 64, 65, 255, 256, 257, 4099, 70001]
TOL, FLOOR = 0.05, 1e-3


def synthetic(content, n):
    """(accumulator [n, 6] float32, samples done, tolerance, floor)."""
    rng = np.random.default_rng(1000 + n)
    k = 2 if content == "k2" else 5
    if content in ("random", "k2", "specials"):
        mu = rng.uniform(0.0, 2.0, (n, 1, 3)).astype(f32)
        sigma = rng.choice(np.array([0.0, 1e-3, 0.03, 0.5], f32), (n, 1, 1))
        L = (mu * (1 + sigma * rng.standard_normal((n, k, 3)).astype(f32))).astype(f32)
        acc = np.zeros((n, 6), f32)
        for i in range(k):   # in-order float32 sums, as the film keeps them
            acc[:, :3] = acc[:, :3] + L[:, i]
            acc[:, 3:] = acc[:, 3:] + L[:, i] * L[:, i]
        if content == "specials":
            kind = rng.integers(0, 8, n)
            acc[kind == 1, 3:] = acc[kind == 1, :3] ** 2 / f32(k) * f32(0.75)   # Q < S²/n: a negative d
            acc[kind == 2] = 0                                                  # nothing seen: M = 0, E = 0
            z = kind == 3                                                       # M = 0, the floor decides
            acc[z, :3] = 0
            acc[z, 3:] = rng.uniform(0, 4e-8, (int(z.sum()), 3)).astype(f32)
            bad = np.array([np.nan, np.inf, -np.inf], f32)
            for row in np.flatnonzero(kind == 4):
                acc[row, rng.integers(0, 6)] = bad[rng.integers(0, 3)]
            acc[kind == 5, 3:] = np.inf
        return acc, k, TOL, FLOOR
    acc = np.empty((n, 6), f32)
    acc[:, :3] = 1.0
    acc[:, 3:] = 10.0 if content == "all_active" else 0.25   # k = 4: d = 9.75, or exactly 0
    if content == "last_only":
        acc[-1, 3:] = 10.0
    if content == "floor_zero":   # M = 0 and floor = 0: T = 0, active iff E > 0
        acc[:, :3] = 0
        acc[:, 3:] = np.where(np.arange(n)[:, None] % 2 == 0, f32(1e-6), f32(0))
        return acc, 4, TOL, 0.0
    return acc, 4, TOL, FLOOR


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("content", ["random", "specials", "k2", "all_active", "none_active", "last_only", "floor_zero"])
def test_select_equals_the_restated_rule(hip, content, n):
    acc_h, k, tol, floor = synthetic(content, n)
    active, E = rule(acc_h, k, tol, floor)
    if content in ("random", "specials", "k2") and n >= 63:
        assert 0 < active.sum() < n, "the content should span both outcomes"
    if content == "all_active":
        assert active.all()
    if content == "none_active":
        assert not active.any()
    if content == "last_only":
        assert active[-1] and active.sum() == 1
    if content == "specials":
        assert np.isfinite(E).sum() > 0 and not np.isnan(E).any()
    acc = torch.from_numpy(acc_h).to(DEV)
    rng = np.random.default_rng(n)
    subset = np.flatnonzero(rng.random(n) < 0.6).astype(np.int32)
    subset = np.union1d(subset, [n - 1]).astype(np.int32)   # ascending, and the last pixel considered
    for listed in (None, subset):
        considered = np.arange(n, dtype=np.int32) if listed is None else listed
        want = considered[active[considered]]
        room = max(1, len(considered))
        out = torch.full((room,), -1, dtype=torch.int32, device=DEV)
        err = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
        lin = None if listed is None else torch.from_numpy(listed).to(DEV)
        torch.cuda.synchronize()
        got_n = hip.adaptive_select(n, k, tol, floor, acc.data_ptr(), out.data_ptr(),
                                    None if lin is None else lin.data_ptr(), 0 if lin is None else lin.numel(),
                                    err.data_ptr())
        out_h, err_h = out.cpu().numpy(), err.cpu().numpy()
        assert got_n == len(want)
        assert np.array_equal(out_h[:got_n], want), "the list: ascending, exactly the active pixels"
        assert (out_h[got_n:] == -1).all(), "list_out was written beyond the active count"
        assert np.array_equal(bits(err_h[considered]), bits(E[considered])), "E of the pixels considered"
        rest = np.ones(n, bool)
        rest[considered] = False
        assert (err_h[rest] == -7.0).all(), "err_out of a pixel that was not considered was written"
        if listed is not None and len(listed) == 0:
            assert got_n == 0


def test_select_without_err_out_and_over_an_empty_list(hip):
    acc_h, k, tol, floor = synthetic("random", 257)
    active, _ = rule(acc_h, k, tol, floor)
    acc = torch.from_numpy(acc_h).to(DEV)
    out = torch.full((257,), -1, dtype=torch.int32, device=DEV)
    lin = torch.zeros((1,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert hip.adaptive_select(257, k, tol, floor, acc.data_ptr(), out.data_ptr()) == active.sum()
    assert np.array_equal(out.cpu().numpy()[:active.sum()], np.flatnonzero(active))
    out.fill_(-1)
    torch.cuda.synchronize()
    assert hip.adaptive_select(257, k, tol, floor, acc.data_ptr(), out.data_ptr(), lin.data_ptr(), 0) == 0
    assert (out == -1).all()


# ------------------------------------------------------------------ 2. a listed pass against the oracle
def some_pixels(npx, row_start, row_len):
    """Every third packed pixel, one whole row, pixels 0 and npx - 1: ascending int32."""
    idx = np.union1d(np.arange(0, npx, 3), np.arange(row_start, row_start + row_len))
    return np.union1d(idx, [0, npx - 1]).astype(np.int32)


def listed_pass(hip, key, s, rd, first, more, listed, stream, what=""):
    """A uniform pass of `first` samples, then a listed pass of `more`; checks listed pixels against the
    oracle at first + more, the rest at first, and that unlisted sums were not written."""
    npx = HipRenderer.n_pixels(rd)
    acc = TP.new_accum(rd)
    torch.cuda.synchronize()
    rgbs, rgbas = TP.passes(hip, rd, 0, first, 1, acc, stream)
    hip.sync()
    rgb, rgba = rgbs[0], rgbas[0]
    before = acc.cpu().numpy().copy()
    lst = torch.from_numpy(np.ascontiguousarray(listed, dtype=np.int32)).to(DEV) if len(listed) else None
    torch.cuda.synchronize()
    hip.render_passes_list(rd, first, more, None if lst is None else lst.data_ptr(), len(listed), acc.data_ptr(),
                           rgb.data_ptr(), rgba.data_ptr(), stream=None if stream is None else stream.cuda_stream)
    plan = hip.last_chunks() if len(listed) else None
    other = torch.cuda.Stream(DEV)
    hip.wait_frame(other.cuda_stream, 0)   # another stream, ordered after the pass
    with torch.cuda.stream(other):
        rgb_o, rgba_o, acc_o = rgb.clone(), rgba.clone(), acc.clone()
    other.synchronize()
    hip.sync()
    torch.cuda.synchronize()
    got, got8, after = rgb.cpu().numpy(), rgba.cpu().numpy(), acc.cpu().numpy()
    assert np.array_equal(bits(rgb_o.cpu().numpy()), bits(got)) and np.array_equal(rgba_o.cpu().numpy(), got8) and \
        np.array_equal(bits(acc_o.cpu().numpy()), bits(after)), f"{what}: wait_frame did not order the copy after the pass"
    lo, lo8 = TP.oracle(key, s, rd, first)
    hi, hi8 = TP.oracle(key, s, rd, first + more)
    on = np.zeros(npx, bool)
    on[listed] = True
    assert np.array_equal(bits(got[on]), bits(hi[on])), f"{what}: listed pixels, float image at {first + more} samples"
    assert np.array_equal(got8[on], hi8[on]), f"{what}: listed pixels, RGBA8 at {first + more} samples"
    assert np.array_equal(bits(got[~on]), bits(lo[~on])), f"{what}: unlisted pixels, float image at {first} samples"
    assert np.array_equal(got8[~on], lo8[~on]), f"{what}: unlisted pixels, RGBA8 at {first} samples"
    assert np.array_equal(bits(after[~on]), bits(before[~on])), f"{what}: an unlisted pixel's sums were written"
    if len(listed) and after[on].any():   # (a list of black pixels only: the sums stay zero)
        assert not np.array_equal(bits(after[on]), bits(before[on])), f"{what}: no listed pixel's sums changed"
    return plan


@pytest.mark.parametrize("sched", ["default", "chunks_3_lanes", "chunks_2_lanes", "serial", "megakernel"])
@pytest.mark.parametrize("kind", sorted(TP.SCENES))
def test_a_listed_pass_equals_the_oracle(hip, kind, sched):
    s, rd = TP.scene(kind)
    W, H = rd.camera.width, rd.camera.height
    hip.upload(s)
    hip.set_schedule(**TP.SCHEDULES[sched])
    listed = some_pixels(W * H, (H // 2) * W, W)
    plan = listed_pass(hip, kind, s, rd, 2, 3, listed, torch.cuda.Stream(DEV), f"{kind}/{sched}")
    hip.set_schedule()
    if sched == "megakernel":
        assert plan["n_chunks"] == 0
    else:   # the plan of a frame of len(listed) pixels
        assert (plan["n_chunks"] - 1) * plan["chunk_pixels"] < len(listed) <= plan["n_chunks"] * plan["chunk_pixels"]


@pytest.mark.parametrize("sched", sorted(TP.FOUR_LANES))
@pytest.mark.parametrize("kind", ["whitted", "path"])
def test_a_listed_pass_on_four_lanes(hip, kind, sched):
    """The four-lane schedules of test_gpu_progressive.py, on a caller's stream (lane 0 then runs on the
    context's stream, joined back before the scatter) and on the context's own."""
    s, rd = TP.scene(kind)
    W, H = rd.camera.width, rd.camera.height
    hip.upload(s)
    hip.set_schedule(**TP.SCHEDULES[sched])
    listed = some_pixels(W * H, (H // 2) * W, W)
    for stream in (torch.cuda.Stream(DEV), None):
        plan = listed_pass(hip, kind, s, rd, 2, 3, listed, stream, f"{kind}/{sched}")
        assert plan["lanes"] == 4
    hip.set_schedule()


def test_a_listed_pass_over_a_rank_shard(hip):
    s, rd = TP.scene("whitted")
    W, H = rd.camera.width, rd.camera.height
    tiles = tiles_for_rank(W, H, 1, 4, 32)
    d = TP.with_spp(rd, 8, tiles=tiles)
    npx = HipRenderer.n_pixels(d)
    w0 = tiles[0][2] - tiles[0][0]
    hip.upload(s)
    hip.set_schedule()
    # (the whole second row of the first tile: runs end at a tile row's end though the packed order goes on)
    listed_pass(hip, "whitted_shard", s, d, 2, 3, some_pixels(npx, w0, w0), torch.cuda.Stream(DEV), "shard")
    # every pixel listed: runs are the tiles' rows
    listed_pass(hip, "whitted_shard", s, d, 2, 3, np.arange(npx, dtype=np.int32), None, "shard, all listed")


@pytest.mark.parametrize("sched", ["default", "megakernel"])
def test_a_list_of_one_pixel_and_an_empty_list(hip, sched):
    s, rd = TP.scene("path")
    W, H = rd.camera.width, rd.camera.height
    hip.upload(s)
    hip.set_schedule(**TP.SCHEDULES[sched])
    listed_pass(hip, "path", s, rd, 2, 3, np.array([(H // 2) * W + W // 2], np.int32), torch.cuda.Stream(DEV), "one pixel")
    listed_pass(hip, "path", s, rd, 2, 3, np.array([], np.int32), torch.cuda.Stream(DEV), "empty list")
    hip.set_schedule()


def test_a_listed_sobol_pass(hip):
    s, rd = scenes.config_c3(96, 54, 8, mesh=TP.small_dragon(40))
    assert rd.sampler == capi.SAMPLER_SOBOL
    W, H = rd.camera.width, rd.camera.height
    hip.upload(s)
    hip.set_schedule()
    listed_pass(hip, "c3_sobol", s, rd, 4, 4, some_pixels(W * H, (H // 2) * W, W), torch.cuda.Stream(DEV), "sobol")


def test_a_listed_sobol_pass_in_the_megakernel_over_wide_indices(hip):
    """The frame of test_sobol_wide_index_pass_over_two_values_of_the_high_bits: the listed pass covers
    samples 128..511, whose index bits >= 32 take two values (0 up to sample 255, 1 from there) — DESIGN §4.2 sends it to the megakernel."""
    s, rd = scenes.config_c3(4096, 8, 512, mesh=TP.small_dragon(24))
    rd2 = scenes.render_desc(rd.camera, rd.integrator, 512, 3, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_SOBOL, tiles=[(2040, 2, 2056, 4)])
    hip.upload(s)
    hip.set_schedule()
    listed = np.array([0, 1, 2, 5, 15, 16, 17, 31], np.int32)
    listed_pass(hip, "c3_wide", s, rd2, 128, 384, listed, None, "wide sobol")
    assert hip.last_chunks()["n_chunks"] == 0


def test_a_bad_list_is_refused(hip):
    s, rd = TP.scene("whitted")
    npx = HipRenderer.n_pixels(rd)
    hip.upload(s)
    hip.set_schedule()
    acc = torch.zeros((npx, 6), dtype=torch.float32, device=DEV)
    rgb = torch.full((npx, 3), -1.0, dtype=torch.float32, device=DEV)
    for bad in ([5, 4, 9], [3, 3], [0, npx], [-1, 2]):
        lst = torch.tensor(bad, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="ascending"):
            hip.render_passes_list(rd, 2, 3, lst.data_ptr(), len(bad), acc.data_ptr(), rgb.data_ptr(), None)
    hip.sync()
    torch.cuda.synchronize()
    assert (rgb == -1.0).all() and (acc == 0).all(), "a refused call rendered"


# ------------------------------------------------------------------ 3. the whole adaptive call
def adaptive(hip, rd, min_samples, per_round, tolerance, floor, stream=None):
    npx = HipRenderer.n_pixels(rd)
    acc = TP.new_accum(rd)
    counts = torch.full((npx,), -1, dtype=torch.int32, device=DEV)
    rgb = torch.full((npx, 3), float("nan"), dtype=torch.float32, device=DEV)
    rgba = torch.zeros((npx, 4), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    res = hip.render_adaptive(rd, min_samples, per_round, tolerance, floor, acc.data_ptr(), counts.data_ptr(),
                              rgb.data_ptr(), rgba.data_ptr(), stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    return res, acc.cpu().numpy(), counts.cpu().numpy(), rgb.cpu().numpy(), rgba.cpu().numpy()


def snapshots_of_passes(hip, rd, ks):
    """The whole-frame accumulator of pbr_hip_render_passes after k samples, for each k in ks (ascending)."""
    acc = TP.new_accum(rd)
    torch.cuda.synchronize()
    snaps, done = {}, 0
    for k in ks:
        TP.passes(hip, rd, done, k - done, 1, acc)
        hip.sync()
        snaps[k] = acc.cpu().numpy().copy()
        done = k
    return snaps


# tolerance per scene: 0.05 unless it leaves no mixed set there (asserted below from the snapshot)
ADAPT_TOL = {"whitted": 0.05, "path": 0.05, "volpath": 0.05}


@pytest.mark.parametrize("sched", ["default", "chunks_3_lanes"])
@pytest.mark.parametrize("kind", sorted(ADAPT_TOL))
def test_adaptive_render_counts_and_images(hip, kind, sched):
    s, rd = TP.scene(kind)
    assert rd.sampler == capi.SAMPLER_HALTON and rd.spp == 8
    npx = HipRenderer.n_pixels(rd)
    tol = ADAPT_TOL[kind]
    hip.upload(s)
    hip.set_schedule(**TP.SCHEDULES[sched])
    snaps = snapshots_of_passes(hip, rd, (2, 4, 6, 8))
    want, first_active = expected_counts(snaps, 2, 2, 8, tol, 1e-3)
    assert 0 < first_active < npx, f"{kind}: tolerance {tol} leaves {first_active} of {npx} active after the first select"
    res, acc, counts, rgb, rgba = adaptive(hip, rd, 2, 2, tol, 1e-3, torch.cuda.Stream(DEV))
    hip.set_schedule()
    assert np.array_equal(counts, want), f"{(counts != want).sum()} pixels with another count"
    assert res.samples == int(counts.sum()) and res.max_samples_done == int(counts.max())
    assert res.rounds == 1 + (int(counts.max()) - 2) // 2   # passes rendered, the full-frame one included
    assert res.active_at_end == int(rule(snaps[int(counts.max())], int(counts.max()), tol, 1e-3)[0][counts == counts.max()].sum())
    for k in (2, 4, 6, 8):
        at = counts == k
        c, c8 = TP.oracle(kind, s, rd, k)
        assert np.array_equal(bits(rgb[at]), bits(c[at])), f"pixels that stopped at {k}: float image"
        assert np.array_equal(rgba[at], c8[at]), f"pixels that stopped at {k}: RGBA8"
        assert np.array_equal(bits(acc[at]), bits(snaps[k][at])), f"pixels that stopped at {k}: sums"


def test_adaptive_counts_from_the_oracles_samples(hip):
    """A 6x4 tile around the dragon, budget 6: the sums come from the oracle's per-sample radiance, added
    in order in float32 (as test_accumulator_holds_the_in_order_sums), and go through the restated rule."""
    s, rd0 = TP.scene("path")
    W, H = rd0.camera.width, rd0.camera.height
    tile = (W // 2 - 3, H // 2 - 2, W // 2 + 3, H // 2 + 2)
    rd = TP.with_spp(rd0, 6, tiles=[tile])
    hip.upload(s)
    hip.set_schedule()
    L = np.array([[O.li_pixel(s, rd, x, y, k) for k in range(6)]
                  for y in range(tile[1], tile[3]) for x in range(tile[0], tile[2])], dtype=f32)   # [24, 6, 3]
    snaps = {}
    acc = np.zeros((24, 6), f32)
    for i in range(6):
        acc[:, :3] = (acc[:, :3] + L[:, i]).astype(f32)
        acc[:, 3:] = (acc[:, 3:] + f32(L[:, i] * L[:, i])).astype(f32)
        snaps[i + 1] = acc.copy()
    for tol in (0.05, 0.2):
        want, _ = expected_counts(snaps, 2, 2, 6, tol, 1e-3)
        res, got_acc, counts, _, _ = adaptive(hip, rd, 2, 2, tol, 1e-3)
        assert np.array_equal(counts, want), f"tolerance {tol}"
        for k in (2, 4, 6):
            assert np.array_equal(bits(got_acc[counts == k]), bits(snaps[k][counts == k]))
        assert res.samples == int(want.sum())


# ------------------------------------------------------------------ 4. limits
def test_limits(hip):
    s, rd = TP.scene("whitted")
    npx = HipRenderer.n_pixels(rd)
    hip.upload(s)
    hip.set_schedule()
    snaps = snapshots_of_passes(hip, rd, (2,))
    two, two8 = TP.oracle("whitted", s, rd, 2)
    # a huge tolerance: every pixel stops at min_samples
    res, acc, counts, rgb, rgba = adaptive(hip, rd, 2, 2, 1e30, 1e-3)
    assert (counts == 2).all() and res.rounds == 1 and res.samples == 2 * npx and res.active_at_end == 0
    assert np.array_equal(bits(rgb), bits(two)) and np.array_equal(rgba, two8) and np.array_equal(bits(acc), bits(snaps[2]))
    # tolerance 0: a pixel goes on while E > 0 (rounds of 3: selects at 2 and 5 samples), one with E == 0 stops
    snaps.update(snapshots_of_passes(hip, rd, (2, 5, 8)))
    want, first_active = expected_counts(snaps, 2, 3, 8, 0.0, 1e-3)
    E = rule(snaps[2], 2, 0.0, 1e-3)[1]
    assert first_active == (E > 0).sum() and 0 < first_active < npx
    res, acc, counts, rgb, rgba = adaptive(hip, rd, 2, 3, 0.0, 1e-3)
    ref, ref8, _ = hip.render(rd)
    assert np.array_equal(counts, want)
    assert (counts[E == 0] == 2).all(), "pixels with E == 0 stop at min_samples"
    up = counts == 8
    # (not every pixel with E > 0 at 2 samples has E > 0 at 5: where a pixel's samples differ by less than
    # float32 resolves in Q - S·m — smooth sky — d is rounding noise of either sign; `want` follows that)
    assert up.any()
    assert np.array_equal(bits(rgb[up]), bits(ref[up])) and np.array_equal(rgba[up], ref8[up]), "at the budget: pbr_hip_render's bits"
    for k in (2, 5):
        c, c8 = TP.oracle("whitted", s, rd, k)
        assert np.array_equal(bits(rgb[counts == k]), bits(c[counts == k])) and np.array_equal(rgba[counts == k], c8[counts == k])
    assert res.max_samples_done == 8 and res.rounds == 3 and res.samples == int(counts.sum())
    # min_samples = the budget: one pass, nothing to decide
    res, acc, counts, rgb, rgba = adaptive(hip, rd, 8, 2, 0.05, 1e-3)
    assert (counts == 8).all() and res.rounds == 1 and res.samples == 8 * npx and res.max_samples_done == 8
    assert np.array_equal(bits(rgb), bits(ref)) and np.array_equal(rgba, ref8)


def test_adaptive_sobol_to_the_budget(hip):
    """Sobol, budget 6 rounded up to 8, rounds of 2 then 4: pixels at 2, 4 and 8 samples have oracle frames."""
    s, rd0 = scenes.config_c3(96, 54, 8, mesh=TP.small_dragon(40))
    rd = TP.with_spp(rd0, 6)
    hip.upload(s)
    hip.set_schedule()
    res, acc, counts, rgb, rgba = adaptive(hip, rd, 4, 4, 0.05, 1e-3)
    assert set(np.unique(counts)) == {4, 8} and res.max_samples_done == 8
    for k in (4, 8):
        c, c8 = TP.oracle("c3_sobol", s, rd0, k)
        assert np.array_equal(bits(rgb[counts == k]), bits(c[counts == k])) and np.array_equal(rgba[counts == k], c8[counts == k])


# ------------------------------------------------------------------ 5. the Python class
def test_adaptive_render_class_checkpoint_and_resume():
    s, rd = TP.scene("path")
    r = HipRenderer(0)
    r.upload(s)
    whole = AdaptiveRender(r, rd, min_samples=2, samples_per_round=2, tolerance=0.05, floor=1e-3)
    rgb, rgba = whole.run()
    want, want8 = rgb.cpu().numpy(), rgba.cpu().numpy()
    end = whole.state()
    assert whole.samples_done == 8 and whole.rounds == 4
    assert np.array_equal(whole.sample_map().cpu().numpy(), end["counts"])
    # the same rounds driven one at a time, checkpointed after two of them and resumed on another renderer
    part = AdaptiveRender(r, rd, min_samples=2, samples_per_round=2, tolerance=0.05, floor=1e-3)
    part.run(max_rounds=2)
    assert part.samples_done == 4 and part.rounds == 2
    saved = part.state()
    rgb_mid = part.run()[0].cpu().numpy()
    assert np.array_equal(bits(rgb_mid), bits(want)), "stepped rounds leave the bits of the one call"
    assert np.array_equal(bits(part.state()["accum"]), bits(end["accum"]))
    r.close()
    r2 = HipRenderer(0)
    r2.upload(s)
    resumed = AdaptiveRender(r2, rd, min_samples=2, samples_per_round=2, tolerance=0.05, floor=1e-3)
    resumed.restore(saved)
    assert resumed.samples_done == 4
    rgb, rgba = resumed.run()
    got = resumed.state()
    assert np.array_equal(got["counts"], end["counts"]) and np.array_equal(bits(got["accum"]), bits(end["accum"]))
    later = end["counts"] > 4   # (pixels sampled after the checkpoint have their image written again)
    assert later.any()
    assert np.array_equal(bits(rgb.cpu().numpy()[later]), bits(want[later]))
    assert np.array_equal(rgba.cpu().numpy()[later], want8[later])
    r2.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(hip):
    s, rd = TP.scene("whitted")
    hip.upload(s)
    hip.set_schedule()
    npx = HipRenderer.n_pixels(rd)
    acc = torch.zeros((npx, 6), dtype=torch.float32, device=DEV)
    rgb = torch.full((npx, 3), -1.0, dtype=torch.float32, device=DEV)
    counts = torch.full((npx,), -1, dtype=torch.int32, device=DEV)
    lst = torch.arange(0, 16, dtype=torch.int32, device=DEV)
    out = torch.full((npx,), -1, dtype=torch.int32, device=DEV)
    n = C.c_int(-5)
    torch.cuda.synchronize()
    lib, INV, UNS = hip.lib, capi.PBR_E_INVALID, capi.PBR_E_UNSUPPORTED

    def select(n_pixels=npx, k=2, tol=0.05, floor=1e-3, accum=acc.data_ptr(), list_out=out.data_ptr(), n_out=C.byref(n)):
        return lib.pbr_hip_adaptive_select(hip.ctx, n_pixels, k, tol, floor, accum, None, 0, list_out, n_out, None)

    assert select(k=1) == INV
    assert select(n_pixels=0) == INV and select(n_pixels=1 << 31) == INV
    assert select(tol=-0.5) == INV and select(tol=float("nan")) == INV
    assert select(floor=-1.0) == INV and select(floor=float("nan")) == INV
    assert select(accum=None) == INV and select(list_out=None) == INV and select(n_out=None) == INV
    assert n.value == -5

    def listed(d, first, samples, lp=lst.data_ptr(), nl=16, accum=acc.data_ptr()):
        return lib.pbr_hip_render_passes_list(hip.ctx, C.byref(d), first, samples, lp, nl, accum, rgb.data_ptr(), None)

    dev = TP.with_spp(rd, 8)
    dev.outputs_on_device = 1
    assert listed(dev, 6, 3) == INV and b"budget" in lib.pbr_hip_last_error(hip.ctx)
    assert listed(dev, 2, 0) == INV and listed(dev, -1, 1) == INV
    assert listed(dev, 2, 1, accum=None) == INV
    assert listed(dev, 2, 1, lp=None) == INV and listed(dev, 2, 1, nl=-1) == INV and listed(dev, 2, 1, nl=npx + 1) == INV
    host = TP.with_spp(rd, 8)
    host.outputs_on_device = 0
    assert listed(host, 2, 1) == INV
    stats = TP.with_spp(rd, 8)
    stats.outputs_on_device, stats.collect_stats = 1, 1
    assert listed(stats, 2, 1) == INV
    table = np.zeros((rd.camera.height, rd.camera.width, 8, 8), dtype=np.float32)
    tab = scenes.render_desc(rd.camera, rd.integrator, 8, rd.max_depth, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_TABLE, sample_table=table)
    tab.outputs_on_device = 1
    assert listed(tab, 2, 1) == UNS

    def whole(d, a, accum=acc.data_ptr(), cnt=counts.data_ptr()):
        return lib.pbr_hip_render_adaptive(hip.ctx, C.byref(d), C.byref(a) if a is not None else None, accum, cnt,
                                           rgb.data_ptr(), None, None)

    A = capi.Adaptive
    assert whole(dev, A(1, 2, 0.05, 1e-3)) == INV and whole(dev, A(9, 2, 0.05, 1e-3)) == INV
    assert b"budget" in lib.pbr_hip_last_error(hip.ctx)
    assert whole(dev, A(2, 0, 0.05, 1e-3)) == INV
    assert whole(dev, A(2, 2, -0.05, 1e-3)) == INV and whole(dev, A(2, 2, float("nan"), 1e-3)) == INV
    assert whole(dev, A(2, 2, 0.05, -1e-3)) == INV and whole(dev, A(2, 2, 0.05, float("nan"))) == INV
    assert whole(dev, None) == INV and whole(dev, A(2, 2, 0.05, 1e-3), accum=None) == INV
    assert whole(dev, A(2, 2, 0.05, 1e-3), cnt=None) == INV
    assert whole(host, A(2, 2, 0.05, 1e-3)) == INV and whole(tab, A(2, 2, 0.05, 1e-3)) == UNS
    with pytest.raises(RuntimeError):   # refused by the library: raised, not ignored
        hip._check(whole(dev, A(9, 2, 0.05, 1e-3)), "render_adaptive")
    hip.sync()
    torch.cuda.synchronize()
    assert (rgb == -1.0).all() and (acc == 0).all() and (counts == -1).all() and (out == -1).all(), "a refused call rendered"
