"""pbr_hip_denoise without a GPU: the export, the struct, every refusal of the two Python wrappers before
a device call, and the numpy restatement of the rule (denoise_expected.py) on frames whose answer is
known: a noise-free frame comes back bit for bit, a noisy one comes back closer to its truth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_expected as DE
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, capi, scenes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbr_hip.h")
INF, NAN = float("inf"), float("nan")
f32 = np.float32


class NoDevice:
    """Stands in for the loaded library: any call through it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")


def renderer_without_device():
    r = HipRenderer.__new__(HipRenderer)
    r.lib = NoDevice()
    r.ctx = C.c_void_p()
    return r


def desc(spp=8, **kw):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_PATH, spp, 3, 1.0, capi.LIGHTS_UNIFORM, capi.SAMPLER_HALTON, **kw)


def test_the_symbol_exists_and_a_null_context_is_rejected():
    lib = capi.load_library()
    p = capi.Denoise(16, 8, 5, 1, 4.0, 0.4, 1.0)
    buf = (C.c_float * 8)()
    a = C.addressof(buf)
    assert lib.pbr_hip_denoise(None, C.byref(p), 8, None, a, a, a, None, None, None) == capi.PBR_E_INVALID


def test_the_struct_matches_the_header():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct pbr_denoise \{(.*?)\} pbr_denoise;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), {"int": C.c_int, "float": C.c_float}[ctype]) for n in names.split(",")]
    assert fields == list(capi.Denoise._fields_)
    assert C.sizeof(capi.Denoise) == 28


GOOD = dict(width=16, height=8, samples=8, accum_ptr=0x1000, aov_ptr=0x2000, rgb_ptr=0x3000)


@pytest.mark.parametrize("change", [
    dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 16, height=1 << 15),
    dict(iterations=0), dict(iterations=9),
    dict(sigma_l=0.0), dict(sigma_l=-1.0), dict(sigma_l=NAN), dict(sigma_n=0.0), dict(sigma_n=NAN), dict(sigma_z=-INF),
    dict(sigma_z=NAN),
    dict(samples=1), dict(samples=0),
    dict(accum_ptr=0), dict(accum_ptr=None), dict(aov_ptr=0), dict(aov_ptr=None),
    dict(rgb_ptr=None), dict(rgb_ptr=0, rgba_ptr=0, var_ptr=0),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_the_wrapper_refuses_bad_arguments_before_any_device_call(change):
    r = renderer_without_device()
    with pytest.raises(ValueError):
        r.denoise(**{**GOOD, **change})


def test_the_wrapper_passes_good_arguments_on():
    """... so the refusals above are the arguments', not the stand-in's: a good call reaches the library
    (samples == 1 is fine when per-pixel counts are given; +inf switches a term off)."""
    r = renderer_without_device()
    for change in (dict(), dict(samples=1, counts_ptr=0x4000), dict(sigma_l=INF, sigma_n=INF, sigma_z=INF),
                   dict(rgb_ptr=None, var_ptr=0x5000), dict(iterations=1), dict(iterations=8)):
        with pytest.raises(AssertionError, match="pbr_hip_denoise was called"):
            r.denoise(**{**GOOD, **change})


def test_progressive_denoise_refuses():
    r = renderer_without_device()
    with pytest.raises(ValueError, match="features=False"):
        ProgressiveRender(r, desc()).denoise()
    p = ProgressiveRender(r, desc(), features=True)
    with pytest.raises(ValueError, match="at least 2 samples"):
        p.denoise()
    p.samples_done = 1
    with pytest.raises(ValueError, match="at least 2 samples"):
        p.denoise()
    p.samples_done = 4
    for bad in (dict(iterations=0), dict(iterations=9), dict(sigma_l=0.0), dict(sigma_n=NAN), dict(sigma_z=-1.0)):
        with pytest.raises(ValueError):
            p.denoise(**bad)
    t = ProgressiveRender(r, desc(tiles=[(0, 0, 8, 8)]), features=True)
    t.samples_done = 4
    with pytest.raises(ValueError, match="tiled"):
        t.denoise()


def two_regions(W=64, H=48, k=8):
    """Noise-free: the left half colour 0.5, normal +z, z = 1; the right half colour 2, normal +x, z = 5;
    albedo 1, variance zero (every sample equals the mean: Q = k L^2, all dyadic)."""
    col = np.where(np.arange(W)[None, :, None] < W // 2, f32(0.5), f32(2.0)) * np.ones((H, W, 3), f32)
    accum = np.concatenate([col * k, col * col * k], -1).reshape(-1, 6).astype(f32)
    aov = np.zeros((H, W, 8), f32)
    aov[..., 0:4] = 1
    left = np.arange(W) < W // 2
    aov[:, left, 6] = 1
    aov[:, left, 7] = 1
    aov[:, ~left, 4] = 1
    aov[:, ~left, 7] = 5
    return accum, aov.reshape(-1, 8), col.reshape(-1, 3)


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6])
def test_a_noise_free_two_region_frame_comes_back_bit_for_bit(levels, demodulate):
    accum, aov, col = two_regions()
    rgb, var = DE.denoise(accum, aov, 64, 48, 8, iterations=levels, demodulate=demodulate)
    assert np.array_equal(rgb.view(np.uint32), col.view(np.uint32))
    assert np.array_equal(var, np.zeros_like(var))


def test_noise_is_reduced_level_by_level():
    """The synthetic frame (sky, textured ramping floor, disc with curved normals; 8 gamma-distributed
    samples): every level count, with and without demodulation, is strictly closer to the truth than the
    input.  With demodulation more levels are closer still (1 > 3 > 5).  Without it the floor's 4 x 3 pixel
    checks are in the filtered signal and the wide levels blur them, so no ordering is asked there: that
    is what demodulation is for."""
    accum, aov, truth = DE.synthetic_frame(64, 48, 8)

    def mse(img):
        return float(((img.astype(np.float64) - truth.astype(np.float64)) ** 2).mean())

    noisy = mse(accum[:, :3] / f32(8))
    errs = {}
    for demod in (False, True):
        for levels in (1, 3, 5):
            rgb, var = DE.denoise(accum, aov, 64, 48, 8, iterations=levels, demodulate=demod)
            assert np.isfinite(rgb).all() and np.isfinite(var).all() and (var >= 0).all()
            errs[demod, levels] = mse(rgb)
    print("noisy", noisy, errs)
    assert all(e < noisy for e in errs.values())
    assert errs[True, 5] < errs[True, 3] < errs[True, 1]


def test_counts_of_zero_and_one_and_a_nan():
    """Per-pixel counts: 0 gives mean 0, 1 gives the sample itself, both variance 0; a NaN colour stays on
    its own pixel."""
    accum, aov, _ = DE.synthetic_frame(16, 12, 8)
    counts = np.full(16 * 12, 8, np.int32)
    counts[5], counts[40] = 0, 1
    x, V, *_ = DE.prepare(accum, aov, 16, 12, 8, counts, demodulate=False)
    assert np.array_equal(x.reshape(-1, 3)[5], np.zeros(3, f32)) and V.reshape(-1)[5] == 0
    assert np.array_equal(x.reshape(-1, 3)[40], accum[40, :3]) and V.reshape(-1)[40] == 0
    accum[77, 0] = NAN
    rgb, var = DE.denoise(accum, aov, 16, 12, 8, counts, iterations=3)
    bad = np.isnan(rgb).any(axis=1)
    assert bad.sum() == 1 and bad[77] and np.isfinite(var).all()


def test_the_film_transform_restated():
    """Known points of the 8-bit transform: black, white (the XYZ round trip leaves 1.0 within rounding),
    the linear toe and clamping."""
    out = DE.film_rgba8(np.array([[0, 0, 0], [1, 1, 1], [0.001, 0.001, 0.001], [9, 9, 9], [-1, -1, -1]], f32))
    assert out[0].tolist() == [0, 0, 0, 255]
    assert out[1].tolist() == [255, 255, 255, 255]
    assert out[2].tolist() == [3, 3, 3, 255]   # 12.92 * 0.001 * 255 + 0.5 = 3.79
    assert out[3].tolist() == [255, 255, 255, 255] and out[4].tolist() == [0, 0, 0, 255]
