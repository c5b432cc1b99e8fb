"""Per-vertex shading normals on the device: hit records against the float32 restatement of the
reference's lines (shading_expected.py) on the bits, and two checks that do not depend on that file —
an analytic identity on a sphere mesh and invariance renders against the oracle — then every render
entry point on the same scene, and that a smooth-shaded sphere mesh is closer to the sphere."""
import ctypes as C

import numpy as np
import pytest
import torch

import aov_expected as E
import oracle_lib as O
import shading_expected as SE
from pysicalbasedraytracer_amd import HipRenderer, capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def query_words(hip, rays):
    """pbr_hip_query's records as float32 words [n, 28] and their int32 view: hit 0, prim 1, b 3:6, p 6:9,
    n 12:15, ns 15:18, dpdu 18:21."""
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
    out = (capi.SurfaceHit * max(1, r.shape[0]))()
    hip._check(hip.lib.pbr_hip_query(hip.ctx, r.shape[0], capi.fptr(r), 0, -1, out), "query")
    assert C.sizeof(capi.SurfaceHit) == 112
    w = np.frombuffer(out, dtype=np.float32).reshape(-1, 28)[:r.shape[0]].copy()
    return w, w.view(np.int32)


def rays_to(origin, targets):
    t = np.asarray(targets, dtype=f32).reshape(-1, 3)
    r = np.empty((t.shape[0], 7), dtype=f32)
    r[:, 0:3] = np.asarray(origin, dtype=f32)
    r[:, 3:6] = t - r[:, 0:3]
    r[:, 6] = np.inf
    return r


# ------------------------------------------------------------------ the scene of tests 4 and 7
XF_A = scenes.compose(scenes.translate(-1.25, 0.1, 0.0),
                      scenes.compose(scenes.rotate_y(35.0), scenes.compose(scenes.rotate_x(-20.0), scenes.scale(0.9, 1.3, 0.7))))
XF_B = scenes.compose(scenes.translate(1.25, -0.1, 0.2),
                      scenes.compose(scenes.rotate_z(25.0), scenes.scale(-1.0, 0.8, 1.1)))   # mirrors: swaps handedness


def standin_scene(normals=True):
    """Two dragon_standin(n=8) copies (128 triangles each) with analytic normals: one under a non-uniform
    scale and two rotations, one under a mirroring transform with reverse=True; a mirror floor, a point
    light and a quad area light.  normals=False: the same scene flat (the oracle takes that one)."""
    P, I, N = scenes.dragon_standin(n=8, normals=True)
    s = scenes.Scene()
    green, red = s.matte((0.2, 0.8, 0.3)), s.matte((0.8, 0.3, 0.2))
    s.mesh(P, I, green, xform=XF_A, normals=N if normals else None)
    s.mesh(P, I, red, xform=XF_B, reverse=True, normals=N if normals else None)
    Pf, If = scenes.quad(-1.5, 6.0)
    s.mesh(Pf, If, s.mirror((0.9, 0.9, 0.9)))
    s.point_light((0.5, 3.0, 3.0), (18.0, 18.0, 18.0))
    Pl, Il = scenes.quad(3.0, 1.0, flip=True)
    s.area_light_mesh(Pl, Il, (6.0, 6.0, 6.0), green)
    return s


CAM = dict(eye=(0.0, 0.6, 4.5), look=(0.0, -0.1, 0.0))


def standin_rays(meshes):
    """Rays from the camera's eye at the meshes' world vertices (shared by up to eight triangles), edge
    midpoints (shared by two) and centroids."""
    tri = meshes.p[:256].astype(np.float64)
    targets = np.concatenate([tri.reshape(-1, 3), (tri[:, [0, 1, 2]] + tri[:, [1, 2, 0]]).reshape(-1, 3) / 2, tri.mean(axis=1)])
    return rays_to(CAM["eye"], targets)


def test_hit_records_equal_the_restatement_bit_for_bit(hip):
    s = standin_scene()
    assert SE.swaps_handedness(XF_B[0]) and not SE.swaps_handedness(XF_A[0])
    hip.upload(s)
    meshes = SE.SceneMeshes(s)
    rays = standin_rays(meshes)
    w, wi = query_words(hip, rays)
    hit = (wi[:, 0] == 1) & (wi[:, 1] < 256)   # (the floor and the light have no normals)
    prim, b = wi[hit, 1], w[hit, 3:6]
    assert hit.sum() > 600 and (prim < 128).sum() > 200 and (prim >= 128).sum() > 200, "both copies are hit"
    assert (b.min(axis=1) < 1e-4).sum() > 100 and (np.sort(b, axis=1)[:, 1] < 1e-4).sum() > 20, "edge and vertex hits"
    want = meshes.expected(prim, b)
    for k, name in enumerate(("n", "ns", "dpdu")):
        got = w[hit, 12 + 3 * k:15 + 3 * k]
        bad = np.flatnonzero((bits(got) != bits(want[:, k])).any(axis=1))
        assert bad.size == 0, f"{name}: {bad.size} of {hit.sum()} records differ, first prim {prim[bad[0]]}: {got[bad[0]]} != {want[bad[0], k]}"
    # the records are smooth-shaded ones: ns is not the facet normal, and n is the facet normal on ns's side
    n, ns = w[hit, 12:15], w[hit, 15:18]
    assert (np.abs(n - ns).max(axis=1) > 1e-3).mean() > 0.9
    assert ((n.astype(np.float64) * ns).sum(axis=1) > -1e-6).all()   # (Faceforward's float32 dot was >= 0)
    # a flat scene's records keep ns == n
    hip.upload(standin_scene(normals=False))
    w0, wi0 = query_words(hip, rays)
    assert np.array_equal(wi0[:, 0:2], wi[:, 0:2]) and same(w0[:, 3:12], w[:, 3:12]), "same hits, b, p, pError"
    assert same(w0[hit, 12:15], w0[hit, 15:18])


# ------------------------------------------------------------------ 5. the analytic identity
def uv_sphere(rows, cols, r):
    """A UV sphere mesh about the origin: float32 vertices near radius r, (rows - 1) * cols * 2 triangles."""
    th = np.linspace(0.0, np.pi, rows + 1)
    ph = np.linspace(0.0, 2 * np.pi, cols + 1)[:-1]
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    P = (r * np.stack([np.sin(T) * np.cos(Ph), np.cos(T), np.sin(T) * np.sin(Ph)], axis=-1)).reshape(-1, 3).astype(f32)
    tris = []
    for i in range(rows):
        for j in range(cols):
            a, b = i * cols + j, i * cols + (j + 1) % cols
            c, d = a + cols, b + cols
            if i > 0:
                tris.append((a, c, b))
            if i < rows - 1:
                tris.append((b, c, d))
    return P, np.asarray(tris, dtype=np.int32)


def test_sphere_mesh_normals_interpolate_to_the_radial_direction(hip):
    """Vertices v on radius r with normals v / r: Σ bᵢ nᵢ = (Σ bᵢ vᵢ) / r = p / r in real arithmetic, so ns is
    normalize(p).  In float32 each side is fewer than 20 roundings of ~6e-8 relative on unit-size values:
    1e-5 absolute.  (r = 2: v / r is exact.)  This does not read shading_expected.py."""
    r = 2.0
    P, I = uv_sphere(12, 16, r)
    N = (P / f32(r)).astype(f32)
    s = scenes.Scene()
    s.mesh(P, I, s.matte((0.5, 0.5, 0.5)), normals=N)
    s.point_light((0.0, 5.0, 5.0), (10.0, 10.0, 10.0))
    hip.upload(s)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = rays_to((0.0, 0.0, 0.0), d)             # from the centre outwards …
    rays[:750, 0:3] = 4.0 * d[:750]                # … and from outside towards the centre
    rays[:750, 3:6] = -d[:750]
    w, wi = query_words(hip, rays)
    assert (wi[:, 0] == 1).all()
    p, ns = w[:, 6:9].astype(np.float64), w[:, 15:18].astype(np.float64)
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    err = float(np.abs(ns - radial).max())
    print(f"max |ns - normalize(p)| = {err:.3g}")
    assert err <= 1e-5
    n = w[:, 12:15].astype(np.float64)
    assert ((n * ns).sum(axis=1) > 0).all(), "n lies on ns's side, whichever way the ray came"
    assert np.abs(n - radial).max() > 1e-2, "the facet normals are not radial: the frame is the interpolated one"


# ------------------------------------------------------------------ 6. invariance against the oracle
UV_MIRRORED = np.array([(0, 0), (-1, 0), (-1, 1)], dtype=f32)   # per triangle: dpdu = p0 - p1, the default's negative


def axis_quad(o, eu, ev):
    """Two triangles (a, b, c), (c, d, a) of the parallelogram o, o + eu, o + eu + ev, o + ev with unshared
    vertices: Triangle::GetUVs' default UVs make each triangle's dpdu = p1 - p0 = ±eu.  Returns (P [6, 3], the
    unit geometric normal eu × ev)."""
    o, eu, ev = (np.asarray(v, dtype=np.float64) for v in (o, eu, ev))
    a, b, c, d = o, o + eu, o + eu + ev, o + ev
    n = np.cross(eu, ev)
    return np.array([a, b, c, c, d, a], dtype=f32), (n / np.linalg.norm(n)).astype(f32)


def box_quads(lo, hi, inward=False, skip=()):
    """The faces of an axis-aligned box as axis_quads, normals outward (inward: a room); skip: faces left out,
    as (axis, side).  Returns (P, I, N) with N the exact axis normal of each vertex's face."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    Ps, Ns = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for side in (0, 1):
            if (k, side) in skip:
                continue
            o = lo.copy()
            o[k] = hi[k] if side else lo[k]
            eu, ev = np.zeros(3), np.zeros(3)
            eu[i], ev[j] = hi[i] - lo[i], hi[j] - lo[j]          # e_i × e_j = e_k
            if (side == 0) != inward:                            # the other orientation
                o, eu, ev = o + eu, -eu, ev
            P, n = axis_quad(o, eu, ev)
            Ps.append(P)
            Ns.append(np.tile(n, (6, 1)))
    P = np.concatenate(Ps)
    return P, np.arange(P.shape[0], dtype=np.int32).reshape(-1, 3), np.concatenate(Ns).astype(f32)


def box_scene(variant, with_normals, integrator, mirrored_uv=False):
    """A 4 × 4 × 4 room open towards the camera, a mirror box, a matte box, a quad area light and a point light;
    VolPath: a material-less box filled with a homogeneous medium.  Every edge length is a power of two and every
    coordinate a small multiple of 0.5, so each edge vector, its length and its reciprocal are exact.

    variant: how the meshes carry their normals, and what the twin without normals does instead.
      geometric  N = the face normal                         twin: the same scene
      negated    N = its negative                            twin: reverse toggled (n must follow ns)
      reversed   reverse=True, N = the face normal           twin: reverse=True (the ts flip); two-sided light
      mirrored   under Scale(-1, 1, 1), N = the face normal  twin: the same transform

    The quad light is one-sided except under `reversed`: Triangle::Sample (Triangle.cpp:372-378) turns the
    sampled point's normal to N's side and reads the orientation flag only for a mesh without normals, while
    Triangle::Intersect's n follows the flag through the ts flip.  A one-sided reversed light with N on its
    unreversed side therefore lights the side it does not show its emission on, which no mesh without normals
    does; with twoSided the side does not enter L, |cos| or the ray offsets, and the frame is the twin's."""
    s = scenes.Scene()
    white, red, mirror = s.matte((0.7, 0.7, 0.7)), s.matte((0.7, 0.2, 0.2)), s.mirror((0.9, 0.9, 0.9))
    xform = scenes.scale(-1.0, 1.0, 1.0) if variant == "mirrored" else None
    sign = f32(-1) if variant == "negated" else f32(1)
    reverse = {"geometric": False, "negated": not with_normals, "reversed": True, "mirrored": False}[variant]
    two_sided = variant == "reversed"

    def add(P, I, N, material, light=None, **kw):
        if with_normals:
            kw["normals"] = (sign * N).astype(f32)
        elif mirrored_uv:
            kw["uv"] = np.tile(UV_MIRRORED, (P.shape[0] // 3, 1))
        if light is not None:
            if "uv" in kw:   # (area_light_mesh takes no UVs: the same calls it makes)
                first = len(s.lights)
                shape = s.mesh(P, I, material, xform=xform, reverse=reverse, area_light_first=first, **kw)
                for t in range(I.shape[0]):
                    l = capi.LightDesc(type=capi.LIGHT_DIFFUSE_AREA, shape=shape, triangle=t, two_sided=int(two_sided), n_samples=1,
                                       medium_inside=-1, medium_outside=-1)
                    l.light_to_world = scenes._xf(xform or scenes.identity())
                    l.Le[:] = [float(c) for c in light]
                    s.lights.append(l)
            else:
                s.area_light_mesh(P, I, light, material, xform=xform, reverse=reverse, two_sided=two_sided, **kw)
        else:
            s.mesh(P, I, material, xform=xform, reverse=reverse, **kw)

    add(*box_quads((-2, -2, -2), (2, 2, 2), inward=True, skip=((2, 1),)), white)
    add(*box_quads((-1.5, -2, -1), (-0.5, -1, 0)), mirror)
    add(*box_quads((0.5, -2, -1.5), (1.5, 0, -0.5)), red)
    Pl, nl = axis_quad((-0.5, 1.5, -0.5), (1, 0, 0), (0, 0, 1))      # x × z = -y: faces down
    add(Pl, np.arange(6, dtype=np.int32).reshape(2, 3), np.tile(nl, (6, 1)), white, light=(8.0, 8.0, 8.0))
    s.point_light((-0.5 if variant == "mirrored" else 0.5, 0.5, 1.5), (6.0, 6.0, 6.0))
    if integrator == capi.INTEGRATOR_VOLPATH:
        med = s.homogeneous_medium(0.2, 0.8, 0.3)
        add(*box_quads((-0.5, -2, 0.5), (0.5, -1, 1.5)), -1, medium_inside=med, medium_outside=-1)
    cam = scenes.camera(40, 32, (0.0, 0.0, 6.5), (0.0, -0.3, 0.0), fov=50.0)
    depth = 5 if integrator == capi.INTEGRATOR_WHITTED else 4
    return s, scenes.render_desc(cam, integrator, 4, depth)


INTEGRATORS = {"whitted": capi.INTEGRATOR_WHITTED, "path": capi.INTEGRATOR_PATH, "volpath": capi.INTEGRATOR_VOLPATH}


@pytest.mark.parametrize("variant", ["geometric", "negated", "reversed", "mirrored"])
@pytest.mark.parametrize("integrator", sorted(INTEGRATORS))
def test_exact_axis_normals_leave_the_oracles_frame(hip, integrator, variant):
    """With the face normal as every vertex's normal the frame arithmetic is exact (unit axis vectors, zeros,
    one exact reciprocal), so the render equals the oracle's render of the twin without normals, as float values
    and in RGBA8 — with one difference that is the reference's own: Triangle.cpp:217 sets ss = Cross(ts, ns) with
    ts = Cross(ss, ns), which is −Normalize(dpdu), not Normalize(dpdu).  Whitted does not see it: Lambert's f does
    not read the tangent, and the mirror's wi = (−wo.x, −wo.y, wo.z) goes back to world space through the same two
    sign changes, exactly.  Path and VolPath draw cosine-distributed directions in the BSDF's frame, and a negated
    tangent turns those by 180° about the normal: the scene without normals is then another Monte Carlo sample
    set, not one ulp away.  For those two integrators the twin therefore carries u-mirrored UVs, (0,0) (−1,0)
    (−1,1) per triangle, which negate its dpdu and change nothing else (no texture reads u, v), and the
    comparison stays exact."""
    integ = INTEGRATORS[integrator]
    mirrored_uv = integ != capi.INTEGRATOR_WHITTED
    s, rd = box_scene(variant, True, integ)
    twin, rd_twin = box_scene(variant, False, integ, mirrored_uv=mirrored_uv)
    assert all(bool(sh.N) for sh in s.shapes) and not any(bool(sh.N) for sh in twin.shapes)
    hip.upload(s)
    g, g8, _ = hip.render(rd)
    c, c8, _ = O.render(twin, rd_twin)
    assert np.isfinite(g).all() and np.unique(c8[:, :3], axis=0).shape[0] > 50, "a frame with content"
    diff = np.flatnonzero((g != c).any(axis=1))
    assert diff.size == 0, f"{diff.size} pixels differ, first {diff[0]}: {g[diff[0]]} != {c[diff[0]]}"
    assert np.array_equal(g8, c8)


def test_the_invariance_scenes_differ_where_they_should(hip):
    """The variants are not vacuous: flipping the light's and the walls' orientation without the twin's
    counterpart changes the frame (so `negated` needs n to follow ns, and `reversed` needs the ts flip)."""
    a, rd = box_scene("geometric", True, capi.INTEGRATOR_WHITTED)
    b, _ = box_scene("reversed", True, capi.INTEGRATOR_WHITTED)
    hip.upload(a)
    ga, _, _ = hip.render(rd)
    hip.upload(b)
    gb, _, _ = hip.render(rd)
    assert not np.array_equal(ga, gb)


# ------------------------------------------------------------------ 7. every entry point, same bits
@pytest.mark.parametrize("integrator", sorted(INTEGRATORS))
def test_megakernel_equals_the_wavefront_schedule(hip, integrator):
    s = standin_scene()
    rd = scenes.render_desc(scenes.camera(48, 32, **CAM), INTEGRATORS[integrator], 4, 4)
    hip.upload(s)
    hip.set_schedule()
    wf, wf8, _ = hip.render(rd)
    hip.set_schedule(kernels=capi.KERNELS_MEGAKERNEL)
    mk, mk8, _ = hip.render(rd)
    hip.set_schedule()
    assert np.isfinite(wf).all()
    assert same(wf, mk) and np.array_equal(wf8, mk8)
    # and the normals are in the picture: the flat scene renders another frame
    hip.upload(standin_scene(normals=False))
    flat, _, _ = hip.render(rd)
    assert not np.array_equal(flat, wf)


def test_passes_cut_3_plus_5_equal_8_whole(hip):
    s = standin_scene()
    rd = scenes.render_desc(scenes.camera(48, 32, **CAM), capi.INTEGRATOR_PATH, 8, 4)
    hip.upload(s)
    npx = 48 * 32

    def buffers():
        return (torch.full((npx, 6), NAN, dtype=torch.float32, device=DEV), torch.full((npx, 3), NAN, dtype=torch.float32, device=DEV),
                torch.zeros((npx, 4), dtype=torch.uint8, device=DEV))

    acc1, rgb1, rgba1 = buffers()
    acc2, rgb2, rgba2 = buffers()
    torch.cuda.synchronize()
    hip.render_passes(rd, 0, 8, acc1.data_ptr(), [rgb1.data_ptr()], [rgba1.data_ptr()])
    hip.render_passes(rd, 0, 3, acc2.data_ptr(), [None], [None])
    hip.render_passes(rd, 3, 5, acc2.data_ptr(), [rgb2.data_ptr()], [rgba2.data_ptr()])
    hip.sync()
    torch.cuda.synchronize()
    assert torch.isfinite(acc1).all()
    assert same(acc1.cpu().numpy(), acc2.cpu().numpy()) and same(rgb1.cpu().numpy(), rgb2.cpu().numpy())
    assert np.array_equal(rgba1.cpu().numpy(), rgba2.cpu().numpy())
    whole, whole8, _ = hip.render(rd)
    assert same(rgb1.cpu().numpy(), whole) and np.array_equal(rgba1.cpu().numpy(), whole8)


def test_the_feature_pass_normal_is_the_hit_records_ns(hip):
    """As test_gpu_aov.py does for flat meshes: the expectation's hits come from the oracle on the flat twin (the
    same geometry), its normals from pbr_hip_query on the uploaded scene."""
    s, flat = standin_scene(), standin_scene(normals=False)
    rd = scenes.render_desc(scenes.camera(48, 32, **CAM), capi.INTEGRATOR_PATH, 4, 4)
    hip.upload(s)
    npx = 48 * 32
    acc = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    img = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.render_aov(rd, 0, 4, acc.data_ptr(), img.data_ptr())
    hip.sync()
    torch.cuda.synchronize()
    want_acc, want_img = E.expected(flat, rd, 0, 4, lambda rays: query_words(hip, rays)[0][:, 15:18])
    assert 0 < want_acc[:, 3].sum() < 4 * npx
    assert same(acc.cpu().numpy(), want_acc) and same(img.cpu().numpy(), want_img)
    hip.upload(flat)
    acc0 = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.render_aov(rd, 0, 4, acc0.data_ptr())
    hip.sync()
    torch.cuda.synchronize()
    a, a0 = acc.cpu().numpy(), acc0.cpu().numpy()
    assert same(a[:, :4], a0[:, :4]) and same(a[:, 7], a0[:, 7]) and not np.array_equal(a[:, 4:7], a0[:, 4:7])


# ------------------------------------------------------------------ 8. it is actually smooth
def test_a_smooth_shaded_sphere_mesh_is_closer_to_the_sphere(hip):
    """A radius-1 16 × 16 UV sphere mesh under a point light, matte, Whitted, 48 × 48: mean absolute error
    against the analytic sphere shape over the pixels all three renders cover fully (the silhouette error is the
    two meshes' alike).  Measured: profiles/shading_normals.md."""
    P, I = uv_sphere(16, 16, 1.0)
    N = P.copy()
    cam = scenes.camera(48, 48, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), fov=50.0)
    rd = scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 8, 3)
    frames, cover = {}, {}
    for name in ("sphere", "flat", "smooth"):
        s = scenes.Scene()
        m = s.matte((0.6, 0.6, 0.6))
        if name == "sphere":
            s.sphere((0.0, 0.0, 0.0), 1.0, m)
        else:
            s.mesh(P, I, m, normals=N if name == "smooth" else None)
        s.point_light((2.0, 3.0, 4.0), (30.0, 30.0, 30.0))
        hip.upload(s)
        frames[name] = hip.render(rd)[0].astype(np.float64)
        img = torch.full((48 * 48, 8), NAN, dtype=torch.float32, device=DEV)
        acc = torch.full((48 * 48, 8), NAN, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        hip.render_aov(rd, 0, 8, acc.data_ptr(), img.data_ptr())
        hip.sync()
        torch.cuda.synchronize()
        cover[name] = img.cpu().numpy()[:, 3] == 1
    inside = cover["sphere"] & cover["flat"] & cover["smooth"]
    assert inside.sum() > 300
    err = {k: float(np.abs(frames[k][inside] - frames["sphere"][inside]).mean()) for k in ("flat", "smooth")}
    print(f"mean |mesh - sphere| over {int(inside.sum())} pixels: flat {err['flat']:.5f}, smooth {err['smooth']:.5f}")
    assert err["smooth"] < err["flat"]
