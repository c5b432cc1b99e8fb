"""pbr_hip_render_passes: a frame's samples in resumable passes over a carried accumulator.

A sample's radiance does not depend on the sampler's spp, and a frame sums a pixel's samples in order
from zero, so the image after k samples has an independent expected value: the oracle's render of the
same descriptor at spp = k (Halton: any k; Sobol: power-of-two k).  Every comparison here is on the
bits (uint32 views), under every schedule, for every integrator; the accumulator itself is checked
against in-order float32 sums of the oracle's per-sample radiance."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
from lane_schedules import assert_regime, four_lanes
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, capi, scenes, tiles_for_rank

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def small_dragon(n=40):
    P, I = scenes.dragon_standin(n=n)
    return P, I, "standin-small"


SCENES = {
    "whitted": lambda: scenes.config_c2(128, 72, 8, mesh=small_dragon(48), sky=scenes.procedural_sky(128, 64)),
    "whitted_lights": lambda: scenes.config_c2_lights(64, 36, 8, mesh=small_dragon(40)),
    "path": lambda: scenes.config_c4(96, 54, 8, mesh=small_dragon(40)),
    "volpath": lambda: scenes.config_c5(80, 45, 8, mesh=small_dragon(40)),
}
SCHEDULES = {
    "default": {},
    "chunks_3_lanes": {"chunk_log2": 12},
    "chunks_2_lanes": {"chunk_log2": 11, "lanes": 2},
    "serial": {"chunk_log2": 12, "serial": True},
    "megakernel": {"kernels": capi.KERNELS_MEGAKERNEL},
}
# Four lanes, each on its own queue (lane_schedules.py).  A pass of 2 samples per pixel is 18,432 /
# 4,608 / 10,368 / 7,200 samples (whitted, whitted_lights, path, volpath): 2^10-sample chunks make 18 /
# 5 / 11 / 8 of them, 2^13 3 / 1 / 2 / 1 (the passes rotate, ordered by pass_order's events).  24 chunks
# need 24,576 samples in a pass: Whitted's passes of 4 samples have 36, Path's and VolPath's one pass
# of 8 has 41 → 40 and 29 → 28; the 64x36 multi-light frame cannot have 24 at all.
FOUR_LANES = four_lanes(more=10, rotating=13, balanced=10)
SCHEDULES.update({name: kw for name, (kw, _) in FOUR_LANES.items()})
PASS_LAYOUT = {(kind, name): ((4, 2) if kind == "whitted" else (8, 1)) if name == "l4_balanced" else (2, 4)
               for kind in SCENES for name in SCHEDULES}   # (samples per pass, passes)
del PASS_LAYOUT[("whitted_lights", "l4_balanced")]

_scene_cache, _oracle_cache = {}, {}


def scene(kind):
    if kind not in _scene_cache:
        _scene_cache[kind] = SCENES[kind]()
    return _scene_cache[kind]


def with_spp(rd, spp, tiles=None, sampler=None, max_depth=None):
    if tiles is None and rd.n_tiles:
        tiles = [(rd.tiles[i].x0, rd.tiles[i].y0, rd.tiles[i].x1, rd.tiles[i].y1) for i in range(rd.n_tiles)]
    return scenes.render_desc(rd.camera, rd.integrator, spp, rd.max_depth if max_depth is None else max_depth,
                              rd.rr_threshold, rd.light_strategy, rd.sampler if sampler is None else sampler, tiles=tiles)


def oracle(key, s, rd, spp):
    """The oracle's frame of `rd` at spp samples per pixel, computed once per (key, spp)."""
    if (key, spp) not in _oracle_cache:
        c, c8, _ = O.render(s, with_spp(rd, spp))
        _oracle_cache[(key, spp)] = (c, c8)
    return _oracle_cache[(key, spp)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def passes(hip, rd, first, per_pass, n, accum, stream=None):
    """One render_passes call with an output pair per pass: (rgb tensors, rgba tensors)."""
    npx = HipRenderer.n_pixels(rd)
    rgbs = [torch.full((npx, 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(n)]
    rgbas = [torch.zeros((npx, 4), dtype=torch.uint8, device=DEV) for _ in range(n)]
    hip.render_passes(rd, first, per_pass, accum.data_ptr(), [t.data_ptr() for t in rgbs], [t.data_ptr() for t in rgbas],
                      stream=None if stream is None else stream.cuda_stream)
    return rgbs, rgbas


def new_accum(rd):
    # NaN: the first pass must not read it
    return torch.full((HipRenderer.n_pixels(rd), 6), float("nan"), dtype=torch.float32, device=DEV)


def check(key, s, rd, k, rgb, rgba, what=""):
    c, c8 = oracle(key, s, rd, k)
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(c)), f"{what}: float image after {k} samples"
    assert np.array_equal(rgba.cpu().numpy(), c8), f"{what}: RGBA8 image after {k} samples"


# ------------------------------------------------------------------ 1. parity per pass
@pytest.mark.parametrize("kind,sched", sorted(PASS_LAYOUT), ids=lambda v: v)
def test_every_pass_equals_the_oracle_at_its_sample_count(hip, kind, sched):
    """Four passes of 2 samples (the balanced four-lane schedule: PASS_LAYOUT), on a caller's stream;
    the four-lane schedules on the context's own stream as well, in the regime they are named for."""
    s, rd = scene(kind)
    per_pass, n = PASS_LAYOUT[(kind, sched)]
    hip.upload(s)
    hip.set_schedule(**SCHEDULES[sched])
    for stream in (torch.cuda.Stream(DEV), None) if sched in FOUR_LANES else (torch.cuda.Stream(DEV),):
        acc = new_accum(rd)
        torch.cuda.synchronize()   # (the NaN fills run on torch's stream, the passes on their own)
        rgbs, rgbas = passes(hip, rd, 0, per_pass, n, acc, stream)
        if sched in FOUR_LANES:
            assert_regime(hip.last_chunks(), FOUR_LANES[sched][1], caller_stream=stream is not None, batch=True)
        hip.sync()
        torch.cuda.synchronize()
        for p in range(n):
            check(kind, s, rd, per_pass * (p + 1), rgbs[p], rgbas[p], f"pass {p}")
    ref, ref8, _ = hip.render(rd)
    assert np.array_equal(bits(rgbs[n - 1].cpu().numpy()), bits(ref))
    assert np.array_equal(rgbas[n - 1].cpu().numpy(), ref8)


@pytest.mark.parametrize("sched", ["default", "chunks_3_lanes"])
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_eight_passes_of_one_sample(hip, kind, sched):
    s, rd = scene(kind)
    hip.upload(s)
    hip.set_schedule(**SCHEDULES[sched])
    stream = torch.cuda.Stream(DEV)
    acc = new_accum(rd)
    rgbs, rgbas = passes(hip, rd, 0, 1, 8, acc, stream)
    hip.sync()
    torch.cuda.synchronize()
    for p in (1, 3, 5, 7):   # (the oracle frames the other tests share)
        check(kind, s, rd, p + 1, rgbs[p], rgbas[p], f"pass {p}")


@pytest.mark.parametrize("sched", ["default", "chunks_3_lanes"])
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_separate_calls_of_3_1_and_4_samples(hip, kind, sched):
    s, rd = scene(kind)
    hip.upload(s)
    hip.set_schedule(**SCHEDULES[sched])
    stream = torch.cuda.Stream(DEV)
    acc = new_accum(rd)
    outs, first = [], 0
    for n in (3, 1, 4):   # queued back to back on one stream, no host wait between them
        outs.append(passes(hip, rd, first, n, 1, acc, stream))
        first += n
    hip.sync()
    torch.cuda.synchronize()
    check(kind, s, rd, 3, outs[0][0][0], outs[0][1][0], "after 3")
    check(kind, s, rd, 4, outs[1][0][0], outs[1][1][0], "after 3 + 1")
    check(kind, s, rd, 8, outs[2][0][0], outs[2][1][0], "after 3 + 1 + 4")


# ------------------------------------------------------------------ 2. accumulator contents
@pytest.mark.parametrize("kind", ["whitted", "path", "volpath"])
def test_accumulator_holds_the_in_order_sums(hip, kind):
    s, rd0 = scene(kind)
    W, H = rd0.camera.width, rd0.camera.height
    tile = (W // 2 - 3, H // 2 - 2, W // 2 + 3, H // 2 + 2)   # 6x4 pixels around the dragon
    rd = with_spp(rd0, 5, tiles=[tile])   # (a budget of 5: each oracle sample rebuilds the scene, 25 ms)
    hip.upload(s)
    L = np.array([[O.li_pixel(s, rd, x, y, k) for k in range(5)]
                  for y in range(tile[1], tile[3]) for x in range(tile[0], tile[2])], dtype=np.float32)   # [24, 5, 3]
    acc = new_accum(rd)
    passes(hip, rd, 0, 2, 1, acc)
    hip.sync()
    mid = acc.cpu().numpy()
    passes(hip, rd, 2, 3, 1, acc)
    hip.sync()
    end = acc.cpu().numpy()
    for got, k in ((mid, 2), (end, 5)):
        s1 = np.zeros((24, 3), np.float32)
        s2 = np.zeros((24, 3), np.float32)
        for i in range(k):
            s1 = (s1 + L[:, i]).astype(np.float32)
            s2 = (s2 + np.float32(L[:, i] * L[:, i])).astype(np.float32)
        assert np.array_equal(bits(got[:, :3]), bits(s1)), f"sums after {k} samples"
        assert np.array_equal(bits(got[:, 3:]), bits(s2)), f"sums of squares after {k} samples"


# ------------------------------------------------------------------ 3. Sobol
def test_sobol_passes_of_1_1_2_and_4(hip):
    s, rd0 = scenes.config_c3(96, 54, 8, mesh=small_dragon(40))
    assert rd0.sampler == capi.SAMPLER_SOBOL
    hip.upload(s)
    stream = torch.cuda.Stream(DEV)
    acc = new_accum(rd0)
    first = 0
    for n in (1, 1, 2, 4):
        rgbs, rgbas = passes(hip, rd0, first, n, 1, acc, stream)
        first += n
        hip.sync()
        check("c3_sobol", s, rd0, first, rgbs[0], rgbas[0], f"after {first}")


@pytest.mark.parametrize("kernels", [capi.KERNELS_AUTO, capi.KERNELS_MEGAKERNEL])
def test_sobol_wide_index_passes(hip, kernels):
    """Sample indices beyond 32 bits (a 4096-wide raster at 512 spp, as test_sobol_wide_index_render): in
    passes 3 and 4 (samples 256..511) the index's bits >= 32 come from the sample number, which the
    pass's pixel-major ids no longer are."""
    s, rd = scenes.config_c3(4096, 8, 512, mesh=small_dragon(24))
    rd2 = scenes.render_desc(rd.camera, rd.integrator, 512, 3, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_SOBOL, tiles=[(2040, 2, 2056, 4)])
    hip.upload(s)
    hip.set_schedule(kernels=kernels)
    acc = new_accum(rd2)
    rgbs, rgbas = passes(hip, rd2, 0, 128, 4, acc, torch.cuda.Stream(DEV))
    hip.sync()
    for p, k in ((0, 128), (1, 256), (3, 512)):
        check("c3_wide", s, rd2, k, rgbs[p], rgbas[p], f"pass {p}")


def test_sobol_wide_index_pass_over_two_values_of_the_high_bits(hip):
    """Passes of 192 and 320 samples of the same frame: the second covers samples 192..511, whose index
    bits >= 32 are 0 up to sample 255 and 1 from there (such a pass runs the megakernel)."""
    s, rd = scenes.config_c3(4096, 8, 512, mesh=small_dragon(24))
    rd2 = scenes.render_desc(rd.camera, rd.integrator, 512, 3, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_SOBOL, tiles=[(2040, 2, 2056, 4)])
    hip.upload(s)
    acc = new_accum(rd2)
    passes(hip, rd2, 0, 192, 1, acc)
    rgbs, rgbas = passes(hip, rd2, 192, 320, 1, acc)
    hip.sync()
    check("c3_wide", s, rd2, 512, rgbs[0], rgbas[0])


# ------------------------------------------------------------------ 4. more samples than a finish slice
def test_passes_longer_than_a_finish_slice(hip):
    """Passes of 4096 and 2048 samples: the finish kernels sum in slices of 2048 and carry across them."""
    s, rd = scenes.config_c3(32, 18, 6144, mesh=small_dragon(24))
    rd2 = scenes.render_desc(rd.camera, rd.integrator, 6144, 3, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_HALTON, tiles=[(15, 10, 17, 11)])
    hip.upload(s)
    acc = new_accum(rd2)
    a, a8 = passes(hip, rd2, 0, 4096, 1, acc)
    b, b8 = passes(hip, rd2, 4096, 2048, 1, acc)
    hip.sync()
    check("c3_slices", s, rd2, 4096, a[0], a8[0])
    check("c3_slices", s, rd2, 6144, b[0], b8[0])


# ------------------------------------------------------------------ 5. tiles
def test_passes_over_a_rank_shard(hip):
    s, rd = scene("whitted")
    W, H = rd.camera.width, rd.camera.height
    tiles = tiles_for_rank(W, H, 1, 4, 32)
    d = with_spp(rd, 8, tiles=tiles)
    npx = sum((t[2] - t[0]) * (t[3] - t[1]) for t in tiles)
    hip.upload(s)
    ref, ref8, _ = hip.render(d)
    acc = new_accum(d)
    assert acc.shape[0] == npx
    rgbs, rgbas = passes(hip, d, 0, 2, 4, acc, torch.cuda.Stream(DEV))
    hip.sync()
    check("whitted_shard", s, d, 4, rgbs[1], rgbas[1])
    assert np.array_equal(bits(rgbs[3].cpu().numpy()), bits(ref))
    assert np.array_equal(rgbas[3].cpu().numpy(), ref8)
    # the accumulator is in the same packed tile order: Σ Li / 8 is the image
    assert np.array_equal(bits(acc.cpu().numpy()[:, :3] / np.float32(8)), bits(ref))


# ------------------------------------------------------------------ 6. checkpoint, variance
def test_checkpoint_resume_and_variance():
    s, rd0 = scenes.config_c3(96, 54, 8, mesh=small_dragon(40))
    rd = with_spp(rd0, 8, sampler=capi.SAMPLER_HALTON)
    r1 = HipRenderer(0)
    r1.upload(s)
    whole = ProgressiveRender(r1, rd)
    for _ in range(4):
        rgb, rgba = whole.step(2)
    r1.sync()
    want, want8 = rgb.cpu().numpy(), rgba.cpu().numpy()
    want_acc = whole.state()["accum"]
    part = ProgressiveRender(r1, rd)
    part.step(2, passes=2)
    assert part.samples_done == 4
    saved = part.state()
    var = part.variance().cpu().numpy()
    mid = saved["accum"]
    r1.close()

    assert np.isfinite(var).all() and (var >= 0).all()
    black = (mid[:, :3] == 0).all(axis=1)   # every sample of the pixel missed: a black background
    assert black.any() and not black.all()
    assert (var[black] == 0).all()
    assert (var[~black] > 0).any()

    r2 = HipRenderer(0)
    r2.upload(s)
    resumed = ProgressiveRender(r2, rd)
    resumed.restore(saved)
    assert resumed.samples_done == 4
    rgb, rgba = resumed.step(4)
    r2.sync()
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(want))
    assert np.array_equal(rgba.cpu().numpy(), want8)
    assert np.array_equal(bits(resumed.state()["accum"]), bits(want_acc))
    ref, ref8, _ = r2.render(rd)
    assert np.array_equal(bits(want), bits(ref)) and np.array_equal(want8, ref8)
    with pytest.raises(ValueError):
        resumed.step(1)   # the budget is spent
    r2.close()


# ------------------------------------------------------------------ 7. wait_frame
def test_wait_frame_orders_another_stream_after_a_pass(hip):
    s, rd = scene("path")
    hip.upload(s)
    hip.set_schedule(chunk_log2=12)
    stream, other = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    acc = new_accum(rd)
    rgbs, rgbas = passes(hip, rd, 0, 2, 4, acc, stream)
    copies = []
    for p in range(4):   # each copy on `other` runs after its pass, whatever the rest of the call does
        hip.wait_frame(other.cuda_stream, p)
        with torch.cuda.stream(other):
            copies.append((rgbs[p].clone(), rgbas[p].clone()))
    other.synchronize()
    hip.sync()
    for p, (c, c8) in enumerate(copies):
        check("path", s, rd, 2 * (p + 1), c, c8, f"copy of pass {p}")


# ------------------------------------------------------------------ 8. refusals
def test_refusals(hip):
    s, rd = scene("whitted")
    hip.upload(s)
    npx = HipRenderer.n_pixels(rd)
    acc = torch.zeros((npx, 6), dtype=torch.float32, device=DEV)
    rgb = torch.full((npx, 3), -1.0, dtype=torch.float32, device=DEV)
    out = (C.c_void_p * 1)(rgb.data_ptr())

    def call(d, first, per_pass, n, accum):
        return hip.lib.pbr_hip_render_passes(hip.ctx, C.byref(d), first, per_pass, n, accum, out, None)

    dev = with_spp(rd, 8)
    dev.outputs_on_device = 1
    assert call(dev, 6, 3, 1, acc.data_ptr()) == capi.PBR_E_INVALID        # past the budget
    assert b"budget" in hip.lib.pbr_hip_last_error(hip.ctx)
    assert call(dev, 0, 3, 3, acc.data_ptr()) == capi.PBR_E_INVALID
    assert call(dev, 0, 0, 1, acc.data_ptr()) == capi.PBR_E_INVALID        # samples_per_pass = 0
    assert call(dev, 0, 1, 0, acc.data_ptr()) == capi.PBR_E_INVALID
    assert call(dev, -1, 1, 1, acc.data_ptr()) == capi.PBR_E_INVALID
    assert call(dev, 0, 1, 1, None) == capi.PBR_E_INVALID                  # accum = NULL
    host = with_spp(rd, 8)
    host.outputs_on_device = 0
    assert call(host, 0, 1, 1, acc.data_ptr()) == capi.PBR_E_INVALID       # host outputs
    table = np.zeros((rd.camera.height, rd.camera.width, 8, 8), dtype=np.float32)
    tab = scenes.render_desc(rd.camera, rd.integrator, 8, rd.max_depth, rd.rr_threshold, rd.light_strategy,
                             capi.SAMPLER_TABLE, sample_table=table)
    tab.outputs_on_device = 1
    assert call(tab, 0, 1, 1, acc.data_ptr()) == capi.PBR_E_UNSUPPORTED    # a table sampler
    with pytest.raises(ValueError):
        hip.render_passes(rd, 0, 1, None, [rgb.data_ptr()])
    with pytest.raises(ValueError):
        hip.render_passes(rd, 4, 5, acc.data_ptr(), [rgb.data_ptr()])
    with pytest.raises(RuntimeError):   # refused by the library: raised, not ignored
        hip._check(call(dev, 6, 3, 1, acc.data_ptr()), "render_passes")
    hip.sync()
    torch.cuda.synchronize()
    assert (rgb == -1.0).all() and (acc == 0).all(), "a refused call rendered"
