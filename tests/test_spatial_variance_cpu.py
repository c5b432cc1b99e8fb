"""The denoiser's spatial variance estimate without a GPU: the exports and the struct, every refusal of the
Python wrappers before a device call, pbr_hip_spatial_variance_host — the device's prepare and estimate
functions compiled for the CPU — against the numpy restatement of the rule (spatial_variance_expected.py) on
the bits, and what the rule implies, checked on the restatement.  The one statistical test says that it is
one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_expected as DE
import spatial_variance_expected as SE
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, TemporalRender, capi, scenes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbr_hip.h")
INF, NAN = float("inf"), float("nan")
f32 = np.float32
SHAPES = ((1, 1), (7, 3), (33, 9), (70, 21))   # one pixel; smaller than the window; one past a tile both ways; several tiles
COUNT_SET = (0, 1, 2, 3, 4, 9)


class NoDevice:
    """Stands in for the loaded library: any call through it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")


def renderer_without_device(lib=None):
    r = HipRenderer.__new__(HipRenderer)
    r.lib = lib if lib is not None else NoDevice()
    r.ctx = C.c_void_p()
    return r


def host():
    """A renderer without a context: spatial_variance_host needs none."""
    return renderer_without_device(capi.load_library())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def desc(spp=8, **kw):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_PATH, spp, 3, 1.0, capi.LIGHTS_UNIFORM, capi.SAMPLER_HALTON, **kw)


def mixed_frame(w, h, seed=None):
    """A synthetic frame (sky: misses with coverage 0 and z 0; floor; disc) whose pixels hold a count drawn from
    COUNT_SET and the sums of that many samples; one NaN and one +inf planted in the sums of frames that have
    room for them.  Returns (accum, aov, counts)."""
    seed = w * 100 + h if seed is None else seed
    rng = np.random.default_rng(seed)
    counts = rng.choice(COUNT_SET, size=w * h).astype(np.int32)
    _, aov, truth = DE.synthetic_frame(w, h, 1, seed=seed)
    accum = np.zeros((w * h, 6), f32)
    for k in COUNT_SET[1:]:
        L = truth[None].astype(np.float64) * rng.gamma(2.0, 0.5, size=(k, w * h, 1))
        sel = counts == k
        accum[sel] = np.concatenate([L.sum(0), (L * L).sum(0)], -1).astype(f32)[sel]
    if w * h >= 20:
        accum[(h // 2) * w + w // 2, 1] = NAN
        accum[(h - 1) * w + 1, 4] = INF
    return accum, aov, counts


# ------------------------------------------------------------------ 1. symbols, struct
def test_the_symbols_exist_and_null_arguments_are_rejected():
    lib = capi.load_library()
    p = capi.Denoise(4, 2, 5, 1, 4.0, 0.4, 1.0)
    sv = capi.SpatialVariance(4, 1)
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    out = (C.c_float * 8)()
    o = C.addressof(out)
    assert lib.pbr_hip_denoise_sv(None, C.byref(p), C.byref(sv), 1, None, a, a, o, None, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_denoise_sv(None, C.byref(p), None, 8, None, a, a, o, None, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_spatial_variance_host(C.byref(p), C.byref(sv), 1, None, a, a, o) == capi.PBR_OK
    assert lib.pbr_hip_spatial_variance_host(C.byref(p), None, 2, None, a, a, o) == capi.PBR_OK
    # the plain call's refusal without sv; samples < 1 with it
    assert lib.pbr_hip_spatial_variance_host(C.byref(p), None, 1, None, a, a, o) == capi.PBR_E_INVALID
    assert lib.pbr_hip_spatial_variance_host(C.byref(p), C.byref(sv), 0, None, a, a, o) == capi.PBR_E_INVALID
    cnt = (C.c_int32 * 8)()
    assert lib.pbr_hip_spatial_variance_host(C.byref(p), C.byref(sv), 0, C.addressof(cnt), a, a, o) == capi.PBR_OK
    assert lib.pbr_hip_spatial_variance_host(None, C.byref(sv), 1, None, a, a, o) == capi.PBR_E_INVALID
    for hole in (4, 5, 6):   # accum, aov, var_out
        args = [C.byref(p), C.byref(sv), 1, None, a, a, o]
        args[hole] = None
        assert lib.pbr_hip_spatial_variance_host(*args) == capi.PBR_E_INVALID, hole
    for mc, r in ((1, 1), (65, 1), (0, 2), (-4, 1), (4, 0), (4, 4), (4, -1)):
        bad = capi.SpatialVariance(mc, r)
        assert lib.pbr_hip_spatial_variance_host(C.byref(p), C.byref(bad), 1, None, a, a, o) == capi.PBR_E_INVALID, (mc, r)
    for mc, r in ((2, 1), (64, 3)):
        good = capi.SpatialVariance(mc, r)
        assert lib.pbr_hip_spatial_variance_host(C.byref(p), C.byref(good), 1, None, a, a, o) == capi.PBR_OK, (mc, r)
    for change in (dict(width=0), dict(height=-1), dict(iterations=0), dict(iterations=9), dict(sigma_n=0.0), dict(sigma_z=NAN)):
        q = capi.Denoise(4, 2, 5, 1, 4.0, 0.4, 1.0)
        for k, v in change.items():
            setattr(q, k, v)
        assert lib.pbr_hip_spatial_variance_host(C.byref(q), C.byref(sv), 1, None, a, a, o) == capi.PBR_E_INVALID, change


def test_the_struct_matches_the_header():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct pbr_spatial_variance \{(.*?)\} pbr_spatial_variance;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), {"int": C.c_int, "float": C.c_float}[ctype]) for n in names.split(",")]
    assert fields == list(capi.SpatialVariance._fields_)
    assert C.sizeof(capi.SpatialVariance) == 8


# ------------------------------------------------------------------ 2. the host twin against the restatement
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
def test_the_host_twin_equals_the_restatement(w, h, demodulate):
    accum, aov, counts = mixed_frame(w, h)
    one = DE.synthetic_frame(w, h, 1, seed=5)
    took = 0
    for radius in (1, 2, 3):
        for min_count in (2, 4):
            for acc, img, k, cnt in ((accum, aov, 0, counts), (one[0], one[1], 1, None)):
                kw = dict(counts=cnt, spatial=(min_count, radius), demodulate=demodulate)
                want = SE.variance(acc, img, w, h, k, **kw)
                got = host().spatial_variance_host(w, h, k, acc, img, **kw)
                assert same(got, want), (f"r {radius}, min_count {min_count}, counts {cnt is not None}: V differs at "
                                         f"{int((bits(got) != bits(want)).sum())} pixels")
                plain = DE.prepare(acc, img, w, h, k, cnt, demodulate)[1].reshape(-1)
                took += int((bits(want) != bits(plain)).sum())
    if w * h > 1:
        assert took > 0, "the estimate should have replaced some pixel's variance"
    # spatial=None: prepare's own V, through the same host function
    got = host().spatial_variance_host(w, h, 0, accum, aov, counts=counts, spatial=None, demodulate=demodulate)
    assert same(got, DE.prepare(accum, aov, w, h, 0, counts, demodulate)[1].reshape(-1))


def test_other_sigmas_reach_the_estimate():
    accum, aov, _ = DE.synthetic_frame(33, 9, 1, seed=2)
    base = SE.variance(accum, aov, 33, 9, 1, spatial=(4, 2))
    for kw in (dict(sigma_n=0.1), dict(sigma_z=0.25), dict(sigma_n=INF, sigma_z=INF)):
        want = SE.variance(accum, aov, 33, 9, 1, spatial=(4, 2), **kw)
        assert same(host().spatial_variance_host(33, 9, 1, accum, aov, spatial=(4, 2), **kw), want), kw
        assert not same(want, base), kw


# ------------------------------------------------------------------ 3. what the rule implies (on the restatement)
def test_counts_at_or_above_min_count_give_the_plain_filter():
    accum, aov, _ = DE.synthetic_frame(40, 30, 4)
    rng = np.random.default_rng(0)
    counts = rng.choice((0, 4, 5, 9), size=40 * 30).astype(np.int32)
    for radius in (1, 3):
        rgb, var = SE.denoise(accum, aov, 40, 30, 0, counts, spatial=(4, radius), iterations=3)
        want = DE.denoise(accum, aov, 40, 30, 0, counts, iterations=3)
        assert same(rgb, want[0]) and same(var, want[1])
    rgb, var = SE.denoise(accum, aov, 40, 30, 4, spatial=(4, 2), iterations=3)
    want = DE.denoise(accum, aov, 40, 30, 4, iterations=3)
    assert same(rgb, want[0]) and same(var, want[1])


def test_a_lone_one_sample_pixel_without_neighbours_keeps_zero():
    """The count-1 pixel is its own region (its normal opposes every neighbour's), so every other tap is dropped
    and the kept taps hold one sample: V stays prepare's 0.  With a like neighbour of count 1 it would not."""
    w, h = 9, 7
    accum = np.zeros((w * h, 6), f32)
    accum[:, :3], accum[:, 3:] = 4 * 0.5, 4 * 0.25 + 1.0   # (noisy enough: Q / k > mean^2)
    aov = np.zeros((w * h, 8), f32)
    aov[:, 0:4] = 1
    aov[:, 6] = 1
    aov[:, 7] = 2
    counts = np.full(w * h, 4, np.int32)
    p = 3 * w + 4
    counts[p] = 1
    accum[p] = (0.75, 0.75, 0.75, 1.0, 1.0, 1.0)
    alone = aov.copy()
    alone[p, 6] = -1
    V = SE.variance(accum, alone, w, h, 0, counts, spatial=(4, 3))
    assert V[p] == 0
    V = SE.variance(accum, aov, w, h, 0, counts, spatial=(4, 3))
    assert V[p] > 0


def test_a_nan_neighbour_reaches_no_other_variance():
    accum, aov, _ = DE.synthetic_frame(24, 16, 1, seed=4)
    p = 9 * 24 + 11
    bad = accum.copy()
    bad[p, 0] = NAN
    for radius in (1, 3):
        V = SE.variance(bad, aov, 24, 16, 1, spatial=(4, radius))
        assert np.isfinite(V).all() and (V >= 0).all()
        clean = SE.variance(accum, aov, 24, 16, 1, spatial=(4, radius))
        near = np.zeros((16, 24), bool)
        near[9 - radius:9 + radius + 1, 11 - radius:11 + radius + 1] = True
        far = ~near.reshape(-1)
        assert same(V[far], clean[far]), "pixels outside the NaN's window are untouched"
        assert not same(V, clean), "pixels inside it pooled one tap fewer"
    # ... and a sum that overflows the moment only (finite colour, infinite u) is dropped the same way
    big = accum.copy()
    big[p, 3] = INF
    V = SE.variance(big, aov, 24, 16, 1, spatial=(4, 2))
    assert np.isfinite(V).all()


def two_regions_one_sample(W=40, H=24):
    """Noise-free, one sample: the left half colour 0.5 at distance 1, the right half colour 2 at distance 5,
    with opposite normals, so that every tap across the border is dropped (e_n alone is 4 / 0.16 = 25); albedo
    1; Q = S^2, all dyadic, so the pooled moments are exact and the estimate is 0."""
    col = np.where(np.arange(W)[None, :, None] < W // 2, f32(0.5), f32(2.0)) * np.ones((H, W, 3), f32)
    accum = np.concatenate([col, col * col], -1).reshape(-1, 6).astype(f32)
    aov = np.zeros((H, W, 8), f32)
    aov[..., 0:4] = 1
    left = np.arange(W) < W // 2
    aov[:, left, 6] = 1
    aov[:, left, 7] = 1
    aov[:, ~left, 6] = -1
    aov[:, ~left, 7] = 5
    return accum, aov.reshape(-1, 8), col.reshape(-1, 3)


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_noise_free_one_sample_frame_comes_back_bit_for_bit(radius, demodulate):
    accum, aov, col = two_regions_one_sample()
    for levels in (1, 3, 5):
        rgb, var = SE.denoise(accum, aov, 40, 24, 1, spatial=(4, radius), iterations=levels, demodulate=demodulate)
        assert same(rgb, col), f"{levels} levels"
        assert np.array_equal(var, np.zeros_like(var))


# ------------------------------------------------------------------ 4. the effect (statistical)
def test_the_estimate_lets_the_filter_work_at_one_sample():
    """Statistical, not on the bits: mean squared error against the truth of the synthetic frame, 5 levels,
    default sigmas, min_count 4.  At one sample per pixel the plain filter returns its input; with the estimate
    the filtered error must be below half of that, for each radius.  The printed table gives the suggested
    radius of the header and of the Python layer (the column with the smallest 1- and 2-sample error)."""
    table = {}
    for k in (1, 2, 4):
        accum, aov, truth = DE.synthetic_frame(64, 48, k, seed=7)
        mse = lambda img: float(((img.astype(np.float64) - truth.astype(np.float64)) ** 2).mean())
        row = [mse(accum[:, :3] / f32(k)), mse(SE.denoise(accum, aov, 64, 48, k, spatial=None)[0]) if k >= 2 else None]
        if k == 1:   # (the plain call refuses one sample; a count of 1 on every pixel is the same frame)
            row[1] = mse(DE.denoise(accum, aov, 64, 48, 0, np.ones(64 * 48, np.int32))[0])
        row += [mse(SE.denoise(accum, aov, 64, 48, k, spatial=(4, r))[0]) for r in (1, 2, 3)]
        table[k] = row
    print("samples  unfiltered  filtered    r=1         r=2         r=3")
    for k, row in table.items():
        print(f"{k:7d}  " + "  ".join(f"{v:.5f}   " for v in row))
    one = table[1]
    # (as it went in up to the rounding of (h x) / h and (x / b) b: a few float32 ulps per pixel)
    assert abs(one[1] - one[0]) <= 1e-5 * one[0], "without the estimate the 1-sample frame comes back as it went in"
    for r in (1, 2, 3):
        assert one[1 + r] < 0.5 * one[1], f"radius {r}: {one[1 + r]} against {one[1]}"
    assert table[4][2:] == [table[4][1]] * 3, "at min_count samples the estimate is not used"
    assert min((1, 2, 3), key=lambda r: one[1 + r]) == 1 and min((1, 2, 3), key=lambda r: table[2][1 + r]) == 1, \
        "the suggested radius (1) is the one with the smallest error here"


# ------------------------------------------------------------------ 5. the wrappers' refusals
GOOD = dict(width=16, height=8, samples=1, accum_ptr=0x1000, aov_ptr=0x2000, rgb_ptr=0x3000, spatial=(4, 1))


@pytest.mark.parametrize("change", [
    dict(spatial=(1, 1)), dict(spatial=(65, 1)), dict(spatial=(0, 1)), dict(spatial=(4, 0)), dict(spatial=(4, 4)),
    dict(spatial=(4, -1)), dict(spatial=(4,)), dict(spatial=4), dict(spatial=(4, 1, 1)), dict(spatial=("a", 1)),
    dict(samples=0), dict(samples=-1),
    dict(spatial=None), dict(spatial=None, samples=0),
    dict(width=0), dict(iterations=9), dict(sigma_n=NAN), dict(accum_ptr=0), dict(rgb_ptr=None),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_the_wrapper_refuses_bad_arguments_before_any_device_call(change):
    r = renderer_without_device()
    with pytest.raises(ValueError):
        r.denoise(**{**GOOD, **change})


def test_the_wrapper_passes_good_arguments_on():
    """... so the refusals above are the arguments', not the stand-in's: with spatial the call reaches
    pbr_hip_denoise_sv (one sample is fine), without it pbr_hip_denoise as before."""
    r = renderer_without_device()
    for change in (dict(), dict(spatial=(2, 3)), dict(spatial=(64, 2)), dict(samples=0, counts_ptr=0x4000), dict(samples=8)):
        with pytest.raises(AssertionError, match="pbr_hip_denoise_sv was called"):
            r.denoise(**{**GOOD, **change})
    with pytest.raises(AssertionError, match="pbr_hip_denoise was called"):
        r.denoise(**{**GOOD, "spatial": None, "samples": 2})


def test_the_host_wrapper_refuses():
    r = renderer_without_device()
    accum, aov, _ = DE.synthetic_frame(8, 4, 1)
    for bad in (dict(spatial=(1, 1)), dict(spatial=(4, 4)), dict(samples=0), dict(spatial=None), dict(sigma_n=0.0),
                dict(accum=None), dict(aov=aov[:5]), dict(counts=np.ones(3, np.int32))):
        kw = {**dict(width=8, height=4, samples=1, accum=accum, aov=aov), **bad}
        with pytest.raises(ValueError):
            r.spatial_variance_host(**kw)


def test_progressive_and_temporal_denoise_refuse():
    r = renderer_without_device()
    p = ProgressiveRender(r, desc(), features=True)
    with pytest.raises(ValueError, match="at least 1 sample"):
        p.denoise(spatial=(4, 1))
    p.samples_done = 1
    with pytest.raises(ValueError, match="at least 2 samples"):
        p.denoise()
    for bad in ((1, 1), (4, 0), (4, 4), (65, 2), 3):
        with pytest.raises(ValueError, match="spatial"):
            p.denoise(spatial=bad)
    t = TemporalRender(r, desc(16), 1)
    with pytest.raises(ValueError, match="no frame yet"):
        t.denoise(spatial=(4, 1))
    t._hist = 0
    for bad in ((1, 1), (4, 0), (4, 4), (65, 2)):
        with pytest.raises(ValueError, match="spatial"):
            t.denoise(spatial=bad)
