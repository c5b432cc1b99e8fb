"""Feature buffers without a GPU: the entry point rejects a NULL context, the Python wrapper validates
before it touches a device, the launch cut (pbr_aov_plan.h, asked through pbr_hip_plan_aov) keeps every
launch below 2^31 samples, and the expected-value helper of the GPU tests (aov_expected.py) gives a
hand-computed case."""
import ctypes as C

import numpy as np
import pytest

import aov_expected as E
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, capi, scenes

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


def desc(spp=8, sampler=capi.SAMPLER_HALTON):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, spp, 3, 1.0, capi.LIGHTS_UNIFORM, sampler)


def test_null_context_is_rejected():
    lib = capi.load_library()
    acc = (C.c_float * 8)()
    rd = desc()
    assert lib.pbr_hip_render_aov(None, C.byref(rd), 0, 1, acc, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_render_aov(None, None, 0, 1, None, None) == capi.PBR_E_INVALID
    assert capi.AOV_CHANNELS == 8


@pytest.mark.parametrize("kw, what", [
    (dict(samples=0), "samples"),
    (dict(first_sample=-1), "first_sample"),
    (dict(accum_ptr=0), "accum"),
    (dict(first_sample=6, samples=3), "budget"),
])
def test_render_aov_validates_before_the_device(kw, what):
    args = dict(first_sample=0, samples=2, accum_ptr=64)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        renderer_without_device().render_aov(desc(), **args)


def test_render_aov_refuses_a_sample_table_and_counts_the_sobol_budget():
    rd = desc(spp=2)
    table = np.zeros(16 * 8 * 2 * 8, dtype=np.float32)
    rd.sampler, rd.sample_table, rd.table_dims = capi.SAMPLER_TABLE, capi.fptr(table), 8
    with pytest.raises(ValueError, match="sample table"):
        renderer_without_device().render_aov(rd, 0, 1, 64)
    with pytest.raises(ValueError, match="budget of 8"):   # Sobol: 5 rounds up to 8
        renderer_without_device().render_aov(desc(spp=5, sampler=capi.SAMPLER_SOBOL), 4, 5, 64)


def test_features_need_the_option():
    p = ProgressiveRender(renderer_without_device(), desc())
    with pytest.raises(ValueError, match="features=False"):
        p.features()


# ------------------------------------------------------------------ the launch cut
def check_cut(n_pixels, samples):
    cut = capi.plan_aov(n_pixels, samples)
    at = 0
    for first, n in cut:   # in order, no gaps, nothing empty
        assert first == at and n >= 1
        assert n * samples < 2 ** 31, (first, n)
        at += n
    assert at == n_pixels
    ppb = 1 if samples >= 256 else 256 // samples
    assert all(n % ppb == 0 for _, n in cut[:-1]), "every launch but the last is whole workgroups"
    return cut


def test_c4_is_cut_below_2_31_samples_per_launch():
    cut = check_cut(3840 * 2160, 1024)   # 8.49 G samples
    assert len(cut) == 4 and cut[0] == (0, (2 ** 31 - 1) // 1024)


def test_one_pixel_one_sample_is_one_launch():
    assert check_cut(1, 1) == [(0, 1)]


@pytest.mark.parametrize("n_pixels", [1, 2, 255, 256, 257, 2304, 1920 * 1080, 2 ** 31 - 1, 2 ** 33 + 5])
@pytest.mark.parametrize("samples", [1, 3, 64, 255, 256, 260, 1024, 2 ** 20, 2 ** 31 - 1])
def test_the_launches_tile_the_pixels(n_pixels, samples):
    if n_pixels * samples >= 2 ** 47:
        return   # (tens of thousands of launches and more: the same loop as the sizes below, only longer)
    check_cut(n_pixels, samples)


def test_the_plan_validates():
    fn = capi.load_library().pbr_hip_plan_aov
    n = C.c_int(7)
    assert fn(0, 1, 0, None, None, C.byref(n)) == capi.PBR_E_INVALID
    assert fn(1, 0, 0, None, None, C.byref(n)) == capi.PBR_E_INVALID
    assert fn(1, 1, 0, None, None, None) == capi.PBR_E_INVALID
    assert fn(1, 1, 1, None, None, C.byref(n)) == capi.PBR_E_INVALID
    assert n.value == 7


# ------------------------------------------------------------------ the expected-value helper
KD = (0.25, 0.5, 0.75)


def quad_case():
    """One matte quad in the plane y = 0 under a pinhole camera 2 above it, looking straight down, fov 90."""
    s = scenes.Scene()
    P, I = scenes.quad(0.0, 10.0)
    s.mesh(P, I, s.matte(KD))
    cam = scenes.camera(4, 4, (0.0, 2.0, 0.0), (0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=90.0)
    return s, scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 3, 1)


def test_the_helper_gives_the_hand_computed_quad():
    s, rd = quad_case()
    acc, img = E.expected(s, rd, 0, 3)
    assert acc.shape == img.shape == (16, 8) and acc.dtype == img.dtype == np.float32
    kd = np.asarray(KD, dtype=f32)
    want = np.zeros(3, dtype=f32)
    for _ in range(3):
        want = (want + kd).astype(f32)
    assert np.array_equal(acc[:, 0:3], np.tile(want, (16, 1)))
    assert np.array_equal(img[:, 0:3], np.tile((want / f32(3)).astype(f32), (16, 1)))
    assert np.array_equal(acc[:, 3], np.full(16, 3, dtype=f32)) and np.array_equal(img[:, 3], np.ones(16, dtype=f32))
    assert np.array_equal(acc[:, 4:7], np.zeros((16, 3), dtype=f32))   # (no normals were given)
    # depth: the plane is 2 along the axis, so a sample's distance is 2 / cos; at fov 90 on a square raster
    # the screen window is [-1, 1]², so pFilm (px, py) is the direction (px / 2 - 1, 1 - py / 2, 1) unnormalised
    import oracle_lib as O
    px = E.packed_pixels(rd)
    q = np.array([(x, y, k, d) for (x, y) in px for k in range(3) for d in range(2)], dtype=np.int32)
    u = O.halton(4, 4, 3, q).astype(np.float64).reshape(16, 3, 2)
    sx = (px[:, None, 0] + u[:, :, 0]) / 2.0 - 1.0
    sy = 1.0 - (px[:, None, 1] + u[:, :, 1]) / 2.0
    t = 2.0 * np.sqrt(1.0 + sx * sx + sy * sy)   # 2 / cos
    centre = [5, 6, 9, 10]
    err = np.abs(img[centre, 7].astype(np.float64) - t.mean(axis=1)[centre]).max()
    assert err <= 1e-6, f"centre depths off by {err:.3g}"
    # and the distances grow outwards
    assert img[[0, 3, 12, 15], 7].min() > img[centre, 7].max()


def test_the_helper_continues_a_carried_sum_in_sample_order():
    s, rd = quad_case()
    whole, img = E.expected(s, rd, 0, 3)
    a, _ = E.expected(s, rd, 0, 1)
    b, img_b = E.expected(s, rd, 1, 2, acc=a)
    assert np.array_equal(b.view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(img_b.view(np.uint32), img.view(np.uint32))


def test_every_albedo_rule():
    s = scenes.Scene()
    m = [s.matte((0.1, -0.5, 2.0)), s.mirror((0.9, 0.8, 0.7)), s.glass(kt=(0.5, 0.6, 0.7)),
         s.metal(eta=(0.2, 0.9, 1.5), k=(3.0, 2.5, 2.0)), s.plastic(kd=(0.3, 0.2, 0.1))]
    alb = [E.material_albedo(s.materials[i]) for i in m]
    assert all(v for _, v in alb)
    assert np.array_equal(alb[0][0], np.array([0.1, 0.0, 2.0], dtype=f32))   # the material's clamp
    assert np.array_equal(alb[1][0], np.array([0.9, 0.8, 0.7], dtype=f32))
    assert np.array_equal(alb[2][0], np.array([0.5, 0.6, 0.7], dtype=f32))
    assert np.array_equal(alb[4][0], np.array([0.3, 0.2, 0.1], dtype=f32))
    eta, k = np.array([0.2, 0.9, 1.5]), np.array([3.0, 2.5, 2.0])
    exact = ((eta - 1) ** 2 + k * k) / ((eta + 1) ** 2 + k * k)
    assert np.abs(alb[3][0] - exact).max() < 1e-6
    assert E.material_albedo(capi.MaterialDesc(type=capi.MAT_NONE)) [1] is False
