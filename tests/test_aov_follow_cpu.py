"""The followed feature pass without a GPU: pbr_hip_mirror_step_host — the function the kernel calls,
compiled for the CPU — against the float32 restatement (aov_follow_expected.mirror_step) on the bits, its
refusals, and the refusals of the Python wrappers before any library call."""
import ctypes as C

import numpy as np
import pytest

import aov_follow_expected as FE
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, TemporalRender, capi, scenes

f32 = np.float32
INF = float("inf")


class NoDevice:
    """Stands in for the loaded library: any call through it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")


def renderer_without_device(lib=None):
    r = HipRenderer.__new__(HipRenderer)
    r.lib = lib if lib is not None else NoDevice()
    r.ctx = C.c_void_p()
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def hits_of(p, perr, n, ns, dpdu, wo):
    """capi.SurfaceHit records holding the fields the step reads."""
    arrs = [np.ascontiguousarray(a, dtype=f32).reshape(-1, 3) for a in (p, perr, n, ns, dpdu, wo)]
    m = arrs[0].shape[0]
    out = (capi.SurfaceHit * max(1, m))()
    for i in range(m):
        h = out[i]
        h.hit, h.prim, h.t = 1, 0, 1.0
        for name, a in zip(("p", "p_error", "n", "ns", "dpdu", "wo"), arrs):
            getattr(h, name)[:] = [float(x) for x in a[i]]
        h.medium_inside = h.medium_outside = -1
    return out, m, arrs


def check(p, perr, n, ns, dpdu, wo, kr, what):
    hits, m, arrs = hits_of(p, perr, n, ns, dpdu, wo)
    kr = np.ascontiguousarray(np.broadcast_to(np.asarray(kr, dtype=f32), (m, 3)))
    got, got_f = renderer_without_device(capi.load_library()).mirror_step_host(hits, kr)
    want, want_f = FE.mirror_step(*arrs, kr)
    assert np.array_equal(got_f, want_f), f"{what}: followed"
    assert same(got, want), f"{what}: rays"
    return want, want_f


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def test_axis_aligned_frames():
    """A mirror in each coordinate plane, seen from both sides: the direction is wo with the normal component
    negated ... exactly, the frame being the axes."""
    eye = np.eye(3, dtype=f32)
    for k in range(3):
        ns, dpdu = eye[k], eye[(k + 1) % 3]
        for side in (1.0, -1.0):
            wo = unit([0.3, -0.5, 0.8])
            wo[k] = abs(wo[k]) * side
            rays, f = check([[1.0, 2.0, 3.0]], [[1e-6, 2e-6, 3e-6]], [ns], [ns], [dpdu], [wo], (0.5, 0.25, 1.0), f"axis {k} side {side}")
            assert f[0] == 1 and rays[0, 6] == INF
            d = rays[0, 3:6]
            want = -wo
            want[k] = wo[k]
            assert same(d, want), (k, side, d, want)
            # the origin left the surface on wo's side (the mirror direction stays on that side)
            assert (rays[0, k] - f32([1.0, 2.0, 3.0])[k]) * side > 0


def random_frames(m, seed):
    rng = np.random.default_rng(seed)
    ns = unit(rng.normal(size=(m, 3)))
    t = rng.normal(size=(m, 3))
    dpdu = (t - (t * ns).sum(1, keepdims=True) * ns).astype(f32) * rng.uniform(0.1, 10.0, size=(m, 1)).astype(f32)
    wo = unit(rng.normal(size=(m, 3)))   # both sides of the surface
    n = np.where(rng.random((m, 1)) < 0.5, ns, -ns).astype(f32)   # (a geometric normal on either side of ns)
    p = rng.uniform(-50.0, 50.0, size=(m, 3)).astype(f32)
    perr = (np.abs(p) * f32(3e-7)).astype(f32)
    kr = rng.uniform(0.0, 1.0, size=(m, 3)).astype(f32)
    return p, perr, n, ns, dpdu, wo, kr


def test_random_frames_on_both_sides():
    p, perr, n, ns, dpdu, wo, kr = random_frames(400, 7)
    rays, f = check(p, perr, n, ns, dpdu, wo, kr, "random frames")
    assert f.all()
    side = (wo * ns).sum(1)
    assert (side > 0).any() and (side < 0).any()
    # a mirror direction: the same angle to ns, on wo's side, and unit length up to rounding
    d = rays[:, 3:6].astype(np.float64)
    assert np.allclose((d * ns).sum(1), side, atol=1e-5) and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)


def test_dpdu_not_orthogonal_to_ns():
    """ss = normalize(dpdu) is then not perpendicular to ns and the frame is skewed; the step uses it as it is."""
    p, perr, n, ns, dpdu, wo, kr = random_frames(300, 11)
    dpdu = (dpdu + ns * f32(0.7)).astype(f32)
    assert (np.abs((unit(dpdu) * ns).sum(1)) > 1e-3).all()
    check(p, perr, n, ns, dpdu, wo, kr, "skewed frames")


def test_wo_in_the_tangent_plane_is_not_followed():
    ns, dpdu = [0.0, 1.0, 0.0], [2.0, 0.0, 0.0]
    wo = [[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.6, 1e-30, 0.8]]
    rays, f = check([[0.0, 0.0, 0.0]] * 4, [[1e-7] * 3] * 4, [ns] * 4, [ns] * 4, [dpdu] * 4, wo, (1.0, 1.0, 1.0), "tangent wo")
    assert f.tolist() == [0, 0, 0, 1]
    assert not rays[:3].any()


def test_black_and_partly_black_kr():
    p, perr, n, ns, dpdu, wo, _ = random_frames(6, 3)
    kr = np.array([(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), (-0.0, 0.0, 0.0), (1, 1, 0)], dtype=f32)
    rays, f = check(p, perr, n, ns, dpdu, wo, kr, "black Kr")
    assert f.tolist() == [0, 1, 1, 1, 0, 1]
    assert not rays[0].any() and not rays[4].any()


def test_the_offset_moves_each_coordinate_up_and_down():
    """Normals along ±x, ±y, ±z with wo on either side: every coordinate of the origin takes the next float
    above and below; a coordinate with no offset is left as it is."""
    cases = []
    for k in range(3):
        for s in (1.0, -1.0):
            for side in (1.0, -1.0):
                nn = np.zeros(3, dtype=f32)
                nn[k] = s
                wo = unit([0.4, 0.5, 0.6])
                wo[k] = abs(wo[k]) * side
                cases.append((nn, np.eye(3, dtype=f32)[(k + 1) % 3], wo))
    n, dpdu, wo = (np.stack([c[j] for c in cases]) for j in range(3))
    p = np.tile(np.asarray([[1.5, -2.5, 0.0]], dtype=f32), (len(cases), 1))
    perr = np.tile(np.asarray([[1e-7, 1e-7, 1e-7]], dtype=f32), (len(cases), 1))
    rays, f = check(p, perr, n, n, dpdu, wo, (1.0, 1.0, 1.0), "offsets")
    assert f.all()
    moved = np.sign(rays[:, 0:3].astype(np.float64) - p.astype(np.float64))
    for k in range(3):
        assert {-1.0, 1.0} <= set(moved[:, k].tolist()), f"coordinate {k} did not move both ways"
        assert 0.0 in set(moved[:, k].tolist())
    # each moved coordinate is at least one float beyond p + offset
    off = np.float64(1e-7)
    for i in range(len(cases)):
        k = int(np.argmax(np.abs(n[i])))
        assert abs(float(rays[i, k]) - float(p[i, k])) > off * 0.999


def test_refusals():
    lib = capi.load_library()
    hits, m, _ = hits_of([[0, 0, 0]], [[0, 0, 0]], [[0, 1, 0]], [[0, 1, 0]], [[1, 0, 0]], [[0, 1, 0]])
    kr, rays, fol = np.ones(3, f32), np.zeros(7, f32), np.zeros(1, np.int32)
    good = [1, hits, kr.ctypes.data, rays.ctypes.data, fol.ctypes.data]
    assert lib.pbr_hip_mirror_step_host(*good) == capi.PBR_OK and fol[0] == 1
    for hole in range(1, 5):
        args = list(good)
        args[hole] = None
        assert lib.pbr_hip_mirror_step_host(*args) == capi.PBR_E_INVALID, hole
    assert lib.pbr_hip_mirror_step_host(-1, *good[1:]) == capi.PBR_E_INVALID
    assert lib.pbr_hip_mirror_step_host(0, *good[1:]) == capi.PBR_OK
    with pytest.raises(ValueError, match="kr for"):
        capi.mirror_step_host(hits, np.ones((2, 3), f32))


def desc(spp=8):
    cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    return scenes.render_desc(cam, capi.INTEGRATOR_PATH, spp, 3, 1.0, capi.LIGHTS_UNIFORM, capi.SAMPLER_HALTON)


@pytest.mark.parametrize("bad", [17, -1])
def test_the_wrappers_refuse_bounces_out_of_range_before_any_library_call(bad):
    r = renderer_without_device()
    with pytest.raises(ValueError, match="mirror_bounces"):
        r.render_aov(desc(), 0, 1, 0x1000, mirror_bounces=bad)
    with pytest.raises(ValueError, match="mirror_bounces"):
        ProgressiveRender(r, desc(), features=True, mirror_bounces=bad)
    with pytest.raises(ValueError, match="mirror_bounces"):
        TemporalRender(r, desc(16), 1, mirror_bounces=bad)


def test_the_wrapper_passes_good_bounces_on():
    """... so the refusals above are the argument's: 0 reaches the plain entry point, 1 and 16 the new one."""
    r = renderer_without_device()
    with pytest.raises(AssertionError, match="pbr_hip_render_aov was called"):
        r.render_aov(desc(), 0, 1, 0x1000)
    for b in (1, 16):
        with pytest.raises(AssertionError, match="pbr_hip_render_aov_mirrors was called"):
            r.render_aov(desc(), 0, 1, 0x1000, mirror_bounces=b)
    assert ProgressiveRender(r, desc(), features=True, mirror_bounces=4).mirror_bounces == 4
    assert TemporalRender(r, desc(16), 1, mirror_bounces=16).mirror_bounces == 16
    assert ProgressiveRender(r, desc()).mirror_bounces == 0 and TemporalRender(r, desc(16), 1).mirror_bounces == 0


def test_the_header_and_the_exports_name_the_new_calls():
    assert capi.AOV_MAX_MIRROR_BOUNCES == 16
    for name in ("pbr_hip_render_aov_mirrors", "pbr_hip_mirror_step_host"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name)
