"""pbr_hip_render_aov_mirrors: the feature pass with mirror bounces followed.

The expected values come from aov_follow_expected.py: the camera rays of aov_expected, each segment's hit
record from pbr_hip_query, the mirror step restated in float32 numpy (pinned against the library's own host
twin in test_aov_follow_cpu.py) and the scene's materials.  Every comparison is on the bits (uint32 views)
unless a docstring says why not."""
import ctypes as C

import numpy as np
import pytest
import torch

import aov_expected as E
import aov_follow_expected as FE
import oracle_lib as O
import ref_scenes as RS
from pysicalbasedraytracer_amd import HipRenderer, PbrError, ProgressiveRender, TemporalRender, capi, scenes
from test_gpu_aov import aov, bits, check, query_words, same, small_dragon, tex_lookup_np, vquad, with_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
NAN = float("nan")
SAMPLERS = {"halton": capi.SAMPLER_HALTON, "sobol": capi.SAMPLER_SOBOL}


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def follow(hip, rd, bounces, first, n, acc=None, image=True, stream=None, lib_call=False):
    """One followed feature pass: (accumulator, image) device tensors; a fresh accumulator is NaN-filled.
    lib_call: through pbr_hip_render_aov_mirrors itself (the wrapper sends 0 bounces to the plain entry point)."""
    npx = HipRenderer.n_pixels(rd)
    if acc is None:
        acc = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    img = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV) if image else None
    torch.cuda.synchronize()
    if lib_call:
        d = hip._device_desc(rd, None if stream is None else stream.cuda_stream)
        hip._check(hip.lib.pbr_hip_render_aov_mirrors(hip.ctx, C.byref(d), int(bounces), first, n, acc.data_ptr(),
                                                      img.data_ptr() if image else None), "render_aov_mirrors")
    else:
        hip.render_aov(rd, first, n, acc.data_ptr(), img.data_ptr() if image else None,
                       stream=None if stream is None else stream.cuda_stream, mirror_bounces=bounces)
    hip.sync()
    torch.cuda.synchronize()
    return acc, img


def query(hip):
    return lambda rays: query_words(hip, rays)


# ------------------------------------------------------------------ the scenes
def xquad(x, y, z0, z1):
    """Two triangles in the plane x = const, |y| <= y, z0 <= z <= z1."""
    P = np.array([(x, -y, z0), (x, -y, z1), (x, y, z1), (x, y, z0)], np.float32)
    return P, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def small_c2():
    return scenes.config_c2(64, 36, 8, mesh=small_dragon(40), sky=scenes.procedural_sky(64, 32))


def corridor():
    """Two facing mirrors x = -1 and x = 1 with different dyadic Kr and a matte wall closing the far end."""
    s = scenes.Scene()
    Pa, Ia = xquad(-1.0, 3.0, -6.0, 3.0)
    s.mesh(Pa, Ia, s.mirror((0.5, 1.0, 0.25)))
    Pb, Ib = xquad(1.0, 3.0, -6.0, 3.0)
    s.mesh(Pb, Ib, s.mirror((1.0, 0.5, 0.5)))
    P = np.array([(-1, -3, -6), (1, -3, -6), (1, 3, -6), (-1, 3, -6)], np.float32)
    s.mesh(P, np.array([(0, 1, 2), (0, 2, 3)], np.int32), s.matte((0.75, 0.5, 0.25)))
    s.point_light((0.0, 0.0, 2.0), (5.0, 5.0, 5.0))
    return s, scenes.render_desc(scenes.camera(64, 36, (0.1, 0.2, 2.5), (0.0, 0.0, -6.0)), capi.INTEGRATOR_WHITTED, 8, 5)


TEX_IMG = (RS.texture_image(16, 8, 3) - f32(0.1)).astype(f32)   # (some texels below 0: the material's clamp shows)
TEX_MAP = (2.0, 1.5, 0.1, -0.2)


def textured_mirror():
    """A Kr-textured mirror patch (gently curved) under the camera, in front of a matte quad it reflects."""
    s = scenes.Scene()
    P, I, UV = RS.uv_patch()
    t = s.image_texture(TEX_IMG, wrap=capi.WRAP_REPEAT, mapping=TEX_MAP)
    s.textures[t].level0 = 1
    s.mesh(P, I, s.set_texture(s.mirror((0.5, 0.5, 0.5)), capi.TEX_KR, t), uv=UV)
    Pq, Iq = vquad(-3.0, 6.0)
    s.mesh(Pq, Iq, s.matte((0.25, 0.5, 0.75)))
    s.point_light((0.0, 4.0, 4.0), (20.0, 20.0, 20.0))
    return s, scenes.render_desc(scenes.camera(40, 24, **RS.CAM_C), capi.INTEGRATOR_PATH, 8, 3)


def textured_albedo(scene):
    """(words, material indices) → albedo: the textured mirror's Kr through its mapping and clamp, else the constants."""
    const = np.stack([E.material_albedo(m)[0] for m in scene.materials])

    def albedo(w, mi):
        su, sv, du, dv = (f32(m) for m in TEX_MAP)
        uv = w[:, FE.W_UV]
        val = np.maximum(tex_lookup_np(TEX_IMG, su * uv[:, 0] + du, sv * uv[:, 1] + dv), f32(0))
        return np.where((mi == 0)[:, None], val, const[mi]).astype(f32)
    return albedo


def deep_mirror_scene():
    """test_stack_depth.deep_scene (the binary walk) with the dragon made a mirror: chains between it and the floor."""
    from test_stack_depth import deep_scene
    s = deep_scene()
    m = capi.MaterialDesc(type=capi.MAT_MIRROR)
    m.Kr[:] = [0.5, 1.0, 0.25]
    s.materials[0] = m
    return s, scenes.render_desc(scenes.camera(16, 9, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0)), capi.INTEGRATOR_WHITTED, 3, 3)


SCENES = {"c2": small_c2, "corridor": corridor, "textured": textured_mirror, "deep": deep_mirror_scene}
_scenes, _values = {}, {}


def scene(kind):
    if kind not in _scenes:
        _scenes[kind] = SCENES[kind]()
    return _scenes[kind]


def values(hip, kind, sampler, bounces, n=8):
    """Per-sample expected values of samples 0..n-1 and the chain statistics, computed once (scene uploaded)."""
    key = (kind, sampler, bounces, n)
    if key not in _values:
        s, rd = scene(kind)
        info = {}
        v = FE.sample_values(query(hip), s, with_(rd, spp=n, sampler=SAMPLERS[sampler]), 0, n, bounces,
                             albedo=textured_albedo(s) if kind == "textured" else None, info=info)
        _values[key] = (v, info)
    return _values[key]


# ------------------------------------------------------------------ 1. parity with the chain expectation
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("kind,bounces", [("c2", 1), ("c2", 4), ("corridor", 1), ("corridor", 2), ("corridor", 3),
                                          ("textured", 2), ("deep", 3)])
def test_parity_with_the_chain_expectation(hip, kind, bounces, sampler):
    s, rd = scene(kind)
    hip.upload(s)
    v, info = values(hip, kind, sampler, bounces)
    steps, fallback, on_mirror = info["steps"], info["fallback"], info["ended_on_mirror"]
    hit = v[:, :, 3] != 0
    if kind == "c2":   # mirror → mesh, mirror → sky (the fallback), direct hits; waves in which only some lanes step
        assert (hit & (steps > 0) & ~fallback).any() and fallback.any() and (hit & (steps == 0) & ~on_mirror).any()
        assert (~hit).any()
    if kind == "corridor":
        assert (on_mirror & (steps == bounces) & ~fallback).any(), "no chain ended at the bound on a mirror"
        if bounces >= 2:
            assert (hit & ~on_mirror & (steps == bounces)).any(), f"no chain reached the wall after {bounces} steps"
    if kind == "textured":
        assert (hit & ~on_mirror & (steps > 0)).any(), "no chain reached the matte quad"
    if kind == "deep":
        assert (steps > 1).any(), "no chain between the mirror dragon and the mirror floor"
        # the upload chose the binary walk, so the pass runs the BINARY instantiation: the packet walk is refused
        probe = np.array([[0.0, 0.55, 2.6, 0.0, -0.3, -1.0, np.inf]], dtype=f32)
        with pytest.raises(PbrError, match="binary form"):   # PBR_E_UNSUPPORTED, as test_deep_tree_walks_and_refusals
            hip.intersect_walk(probe, capi.WALK_PACKET)
        assert hip.intersect_walk(probe, capi.WALK_BINARY).shape == (1, 5)
    hip.set_profiling(2)   # (2: with the work counters the families' bytes are formed from)
    for spp in (1, 3, 8):
        acc, img = follow(hip, with_(rd, spp=spp, sampler=SAMPLERS[sampler]), bounces, 0, spp)
        check(acc, img, E.accumulate(v[:, :spp]), spp, f"{kind} B={bounces} {sampler} {spp} spp")
    prof = hip.get_profile()
    hip.set_profiling(False)
    fam = "k_aov_follow_tex" if kind == "textured" else "k_aov_follow"   # the instantiation taken, by its profile family
    other = {"k_aov", "k_aov_tex", "k_aov_follow", "k_aov_follow_tex"} - {fam}
    assert fam in prof and not (other & set(prof)), sorted(prof)
    assert prof[fam]["launches"] == 3 and prof[fam]["bytes"] == 32 * 2 * HipRenderer.n_pixels(rd) * 3


def test_following_changes_the_mirror_pixels(hip):
    """... so the parity above is not that of the plain pass: on the C2 floor the followed pass differs."""
    s, rd = scene("c2")
    hip.upload(s)
    rd1 = with_(rd, spp=1, sampler=capi.SAMPLER_HALTON)
    a0, _ = aov(hip, rd1, 0, 1)
    a1, _ = follow(hip, rd1, 1, 0, 1)
    a0, a1 = a0.cpu().numpy(), a1.cpu().numpy()
    assert not same(a0, a1) and same(a0[:, 3], a1[:, 3])   # (a mirror hit stays a hit: the fallback)
    assert (a1[:, 7] >= a0[:, 7]).all()


def test_one_pixel_one_sample_steps_once(hip):
    """A 1×1 frame at 1 sample: one lane of one wave is live, and it steps."""
    s, rd = scene("corridor")
    hip.upload(s)
    cam = scenes.camera(1, 1, (0.0, 0.0, 2.5), (1.0, 0.0, 0.5), fov=10.0)   # (the whole pixel lies on the mirror x = 1)
    rd1 = with_(rd, spp=1, sampler=capi.SAMPLER_HALTON, camera=cam)
    info = {}
    want, _ = FE.expected(query(hip), s, rd1, 0, 1, 1, info=info)
    assert info["steps"].tolist() == [[1]] and want[0, 3] == 1
    acc, img = follow(hip, rd1, 1, 0, 1)
    check(acc, img, want, 1, "1x1")


def test_a_pixel_of_two_folding_rounds(hip):
    """260 samples per pixel: the pixel is alone in its workgroup and its sums are carried over two rounds."""
    s, rd = scene("c2")
    hip.upload(s)
    cam = scenes.camera(8, 4, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    rd2 = with_(rd, spp=260, sampler=capi.SAMPLER_HALTON, camera=cam)
    info = {}
    want, _ = FE.expected(query(hip), s, rd2, 0, 260, 2, info=info)
    assert (info["steps"] > 0).any()
    acc, img = follow(hip, rd2, 2, 0, 260)
    check(acc, img, want, 260, "260 spp")


# ------------------------------------------------------------------ 2. max_bounces = 0
def test_zero_bounces_is_the_plain_pass(hip):
    for kind, mk in (("c2", small_c2), ("c4", lambda: scenes.config_c4(64, 36, 8, mesh=small_dragon(40)))):
        s, rd = mk()
        hip.upload(s)
        rd3 = with_(rd, spp=3, sampler=capi.SAMPLER_HALTON)
        plain, plain_img = (t.cpu().numpy() for t in aov(hip, rd3, 0, 3))
        hip.set_profiling(True)
        zero, zero_img = (t.cpu().numpy() for t in follow(hip, rd3, 0, 0, 3, lib_call=True))
        prof = hip.get_profile()
        hip.set_profiling(False)
        assert same(zero, plain) and same(zero_img, plain_img), kind
        assert "k_aov" in prof and "k_aov_follow" not in prof and prof["k_aov"]["launches"] == 1, sorted(prof)
        if kind == "c4":   # no mirror material: following finds nothing to follow
            four, four_img = (t.cpu().numpy() for t in follow(hip, rd3, 4, 0, 3))
            assert same(four, plain) and same(four_img, plain_img)


def test_bounces_out_of_range_are_refused(hip):
    s, rd = scene("corridor")
    hip.upload(s)
    acc = torch.zeros((HipRenderer.n_pixels(rd), 8), dtype=torch.float32, device=DEV)
    d = hip._device_desc(rd, None)
    for bad in (-1, 17):
        assert hip.lib.pbr_hip_render_aov_mirrors(hip.ctx, C.byref(d), bad, 0, 1, acc.data_ptr(), None) == capi.PBR_E_INVALID
    assert hip.lib.pbr_hip_render_aov_mirrors(hip.ctx, C.byref(d), 16, 0, 1, acc.data_ptr(), None) == capi.PBR_OK
    hip.sync()


# ------------------------------------------------------------------ 3. passes
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_any_cut_into_passes_leaves_the_same_bits(hip, sampler):
    s, rd = scene("c2")
    hip.upload(s)
    rd8 = with_(rd, spp=8, sampler=SAMPLERS[sampler])
    one, one_img = follow(hip, rd8, 4, 0, 8)
    assert torch.isfinite(one).all() and torch.isfinite(one_img).all()
    for cut in ((2, 3, 3), (1,) * 8, (5, 3)):
        acc, img, at = None, None, 0
        for n in cut:
            acc, img = follow(hip, rd8, 4, at, n, acc)
            at += n
        assert same(acc.cpu().numpy(), one.cpu().numpy()), f"accumulator after {cut}"
        assert same(img.cpu().numpy(), one_img.cpu().numpy()), f"image after {cut}"


# ------------------------------------------------------------------ 4. medium boundaries
def boundary_scene(box):
    """A mirror floor reflecting a wall; the material-less box stands between them, off the camera's direct view
    of the wall's upper part."""
    s = scenes.Scene()
    Pf, If = scenes.quad(0.0, 40.0)
    s.mesh(Pf, If, s.mirror((0.5, 1.0, 0.25)))
    Pw, Iw = vquad(-5.0, 40.0)
    s.mesh(Pw, Iw, s.matte((0.3, 0.6, 0.9)))
    if box:
        Pb, Ib = RS.box((-1.0, 0.2, -3.5), (1.0, 1.2, -2.5))
        s.mesh(Pb, Ib, -1)   # no material: a medium interface
    s.point_light((0.0, 3.0, 2.0), (5.0, 5.0, 5.0))
    return s, scenes.render_desc(scenes.camera(32, 32, (0.0, 1.0, 3.0), (0.0, 0.5, -5.0), fov=60.0), capi.INTEGRATOR_PATH, 3, 3)


def test_material_less_faces_between_a_mirror_and_what_it_reflects(hip):
    """Channels 0-6 on the bits; the distance within 1e-5 relative: the bound and margin of
    test_material_less_faces_are_passed_through (two crossings, each moving the origin by a few ulp of |p|)."""
    plain, rd = boundary_scene(False)
    hip.upload(plain)
    a0, i0 = (t.cpu().numpy() for t in follow(hip, rd, 1, 0, 3))
    first, _ = aov(hip, rd, 0, 3)
    boxed, _ = boundary_scene(True)
    hip.upload(boxed)
    a1, i1 = (t.cpu().numpy() for t in follow(hip, rd, 1, 0, 3))
    assert np.array_equal(a0[:, 3], np.full(32 * 32, 3, dtype=f32))
    assert same(a1[:, :7], a0[:, :7]) and same(i1[:, :7], i0[:, :7])
    moved = a1[:, 7] != a0[:, 7]
    floor = np.abs(first.cpu().numpy()[:, 5]) == 3   # (the plain pass's ns.y sums to ±3 where all three samples see the floor)
    assert (moved & floor).any(), "no reflected ray crossed the box"
    rel = float(np.abs(a1[:, 7].astype(np.float64) / a0[:, 7].astype(np.float64) - 1.0).max())
    rel_img = float(np.abs(i1[:, 7].astype(np.float64) / i0[:, 7].astype(np.float64) - 1.0).max())
    print(f"distance through the box: {rel:.3g} (sums), {rel_img:.3g} (image) relative")
    assert rel <= 1e-5 and rel_img <= 1e-5, f"distance through the box off by {rel:.3g} (sums), {rel_img:.3g} (image) relative"


# ------------------------------------------------------------------ 5. the unfolded twin
def wall(y0):
    P = np.array([(-100, y0, -5), (100, y0, -5), (100, 100, -5), (-100, 100, -5)], np.float32)
    return P, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def twin(folded):
    """A: a mirror floor y = 0 (Kr 1) and a matte wall z = -5 above it.  B: no floor, the wall continued to
    y = -100 with the same winding: the mirror image joined to the original."""
    s = scenes.Scene()
    if folded:
        Pf, If = scenes.quad(0.0, 100.0)
        s.mesh(Pf, If, s.mirror((1.0, 1.0, 1.0)))
    Pw, Iw = wall(0.0 if folded else -100.0)
    s.mesh(Pw, Iw, s.matte((0.3, 0.6, 0.9)))
    s.point_light((0.0, 3.0, 2.0), (5.0, 5.0, 5.0))
    return s


def twin_camera(dx=0.0):
    return scenes.camera(64, 36, (dx, 1.0, 3.0), (dx, 0.5, -5.0))


def twin_desc(cam):
    return scenes.render_desc(cam, capi.INTEGRATOR_PATH, 1, 3, sampler=capi.SAMPLER_HALTON)


def test_the_unfolded_twin(hip):
    """A followed once against B plain: channels 0-6 on the bits, the distance within 1e-4 relative.  A and B differ
    by offset_ray_origin's few-ulp shift of the continuation's origin and one more float addition, about 1e-6
    relative; the bound is a hundred times that."""
    rd = twin_desc(twin_camera())
    hip.upload(twin(True))
    a, ai = (t.cpu().numpy() for t in follow(hip, rd, 1, 0, 1))
    a_first, _ = aov(hip, rd, 0, 1)
    hip.upload(twin(False))
    b, bi = (t.cpu().numpy() for t in aov(hip, rd, 0, 1))
    assert np.array_equal(ai[:, 3], np.ones(64 * 36, f32)) and np.array_equal(bi[:, 3], np.ones(64 * 36, f32)), "coverage"
    floor = a_first.cpu().numpy()[:, 5] != 0
    assert floor.any() and not floor.all()
    assert same(a[:, :7], b[:, :7]) and same(ai[:, :7], bi[:, :7])
    rel = np.abs(ai[:, 7].astype(np.float64) / bi[:, 7].astype(np.float64) - 1.0)
    print(f"unfolded twin: distance off by at most {rel.max():.3g} relative ({rel[floor].max():.3g} on the floor)")
    assert rel.max() <= 1e-4
    assert not same(ai[floor, 7], a_first.cpu().numpy()[floor, 7])


# ------------------------------------------------------------------ 6. the reprojection consequence
def motion_of(hip, scene_, bounces):
    """motion_out of pbr_hip_temporal between the cameras at x = 0 (previous) and x = 0.5 (current), each frame
    with its own sums and features of `scene_` at 1 sample."""
    hip.upload(scene_)
    n = 64 * 36
    frames = []
    for dx in (0.0, 0.5):
        cam = twin_camera(dx)
        rd = twin_desc(cam)
        acc = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        hip.render_passes(rd, 0, 1, acc.data_ptr(), [None], [None])
        _, img = follow(hip, rd, bounces, 0, 1)
        frames.append((acc, img, capi.camera_matrices(cam, hip.lib)))
    (pacc, pimg, pcam), (cacc, cimg, ccam) = frames
    ones = torch.ones((n,), dtype=torch.int32, device=DEV)
    out, cnt = torch.zeros_like(cacc), torch.zeros_like(ones)
    motion = torch.full((n, 2), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.temporal(64, 36, 1, cacc.data_ptr(), cimg.data_ptr(), ones.data_ptr(), pacc.data_ptr(), pimg.data_ptr(),
                 out.data_ptr(), cnt.data_ptr(), ccam, pcam, motion_ptr=motion.data_ptr(), max_history=8)
    hip.sync()
    torch.cuda.synchronize()
    return motion.cpu().numpy(), cimg.cpu().numpy()


def test_reflections_reproject_with_the_parallax_of_the_virtual_point(hip):
    """The motion of A followed equals B's within 1e-2 pixel on every pixel (a depth error of 1e-4 relative moves the
    projection by about 1e-4 pixel here); the motion of A unfollowed misses it by more than a pixel on the floor:
    W / (2 tan(fov / 2)) · b · (1 / z_f - 1 / z_v) = 32 · 0.5 · (1 / z_f - 1 / z_v) pixels."""
    mb, _ = motion_of(hip, twin(False), 0)
    ma, _ = motion_of(hip, twin(True), 1)
    m0, img0 = motion_of(hip, twin(True), 0)
    assert np.isfinite(mb).all() and np.abs(mb).max() > 1, "the cameras should be a pixel or more apart"
    err = np.abs(ma - mb).max(axis=1)
    miss = np.abs(m0 - mb).max(axis=1)
    floor = img0[:, 5] != 0
    print(f"motion, followed against the twin: {err.max():.3g} px; unfollowed: {miss[floor].max():.3g} px on the floor")
    assert err.max() <= 1e-2
    assert floor.any() and miss[floor].max() > 1.0
    assert miss[~floor].max() <= 1e-2   # (the wall seen directly: only B's taller triangles differ, in the last bits of t)


# ------------------------------------------------------------------ 7. bystanders
def test_renders_and_passes_are_unchanged_by_followed_passes(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd4 = with_(rd, spp=4, sampler=capi.SAMPLER_HALTON)
    v, _ = values(hip, "c2", "halton", 4)
    want_acc = E.accumulate(v[:, :4])
    c, c8, _ = O.render(s, rd4)
    follow(hip, rd4, 4, 0, 4)
    g, g8, _ = hip.render(rd4)
    assert same(g, c) and np.array_equal(g8, c8), "render after a followed pass"
    npx = HipRenderer.n_pixels(rd4)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    pacc = torch.full((npx, 6), NAN, dtype=torch.float32, device=DEV)
    rgb = torch.full((npx, 3), NAN, dtype=torch.float32, device=DEV)
    rgba = torch.zeros((npx, 4), dtype=torch.uint8, device=DEV)
    facc = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    fimg = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.render_passes(rd4, 0, 2, pacc.data_ptr(), [None], [None], stream=s1.cuda_stream)
    hip.render_aov(rd4, 0, 4, facc.data_ptr(), fimg.data_ptr(), stream=s2.cuda_stream, mirror_bounces=4)
    hip.render_passes(rd4, 2, 2, pacc.data_ptr(), [rgb.data_ptr()], [rgba.data_ptr()], stream=s1.cuda_stream)
    hip.sync()
    torch.cuda.synchronize()
    assert same(rgb.cpu().numpy(), c) and np.array_equal(rgba.cpu().numpy(), c8), "passes around a followed pass"
    check(facc, fimg, want_acc, 4, "followed pass between two passes")


def test_progressive_render_follows_and_round_trips(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd8 = with_(rd, spp=8, sampler=capi.SAMPLER_HALTON)
    v, _ = values(hip, "c2", "halton", 4)
    want_acc = E.accumulate(v)
    want = E.image(want_acc, 8)
    one = ProgressiveRender(hip, rd8, features=True, mirror_bounces=4)
    rgb1, _ = one.step(8)
    f1 = {k: t.cpu().numpy() for k, t in one.features().items()}
    assert same(f1["albedo"], want[:, 0:3]) and same(f1["coverage"], want[:, 3])
    assert same(f1["normal"], want[:, 4:7]) and same(f1["depth"], want[:, 7])
    a = ProgressiveRender(hip, rd8, features=True, mirror_bounces=4)
    a.step(2)
    a.step(3)
    st = a.state()
    b = ProgressiveRender(hip, rd8, features=True, mirror_bounces=4)
    b.restore(st)
    rgb2, _ = b.step(3)
    assert same(rgb2.cpu().numpy(), rgb1.cpu().numpy())
    assert same(b.state()["features"], want_acc)
    plain = ProgressiveRender(hip, rd8, features=True)
    plain.step(8)
    assert not same(plain.state()["features"], want_acc)


def test_temporal_render_follows(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd16 = with_(rd, spp=16, sampler=capi.SAMPLER_HALTON)
    t = TemporalRender(hip, rd16, 2, cycle=8, mirror_bounces=4)
    cams = [scenes.camera(64, 36, (0.05 * f, 0.55, 2.6), (0.05 * f, -0.25, 0.0)) for f in range(3)]
    for cam in cams:
        t.frame(cam)
    torch.cuda.synchronize()
    got = t.history()["features"].cpu().numpy()
    rd_last = with_(rd16, camera=cams[-1])
    zeros = lambda: torch.zeros((64 * 36, 8), dtype=torch.float32, device=DEV)
    acc = follow(hip, rd_last, 4, 4, 2, acc=zeros(), image=False)[0].cpu().numpy()   # (frame 2 draws samples 4 and 5)
    assert same(got, E.image(acc, 2)), "the feature image of the last frame"
    plain = aov(hip, rd_last, 4, 2, acc=zeros())[0].cpu().numpy()
    assert not same(acc, plain)
