"""pbr_hip_render_aov: feature buffers — per pixel the albedo, coverage, shading normal and distance of
the first surface each camera sample sees, summed in sample order over a carried accumulator.

The expected values come from aov_expected.py (the oracle's sampler, camera and intersection, the
scene's materials, float32 numpy) and, for the shading normal, from pbr_hip_query on the same rays.
Every comparison is on the bits (uint32 views) unless a docstring says why not."""
import numpy as np
import pytest
import torch

import aov_expected as E
import oracle_lib as O
import ref_scenes as RS
from parity import assert_parity
from pysicalbasedraytracer_amd import HipRenderer, PbrError, ProgressiveRender, assemble, capi, scenes, tiles_for_rank

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def small_dragon(n=40):
    P, I = scenes.dragon_standin(n=n)
    return P, I, "standin-small"


def vquad(z, half):
    """Two coplanar triangles in the plane z, facing +z."""
    P = np.array([(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)], np.float32)
    return P, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


SCENES = {
    "c2": lambda: scenes.config_c2(64, 36, 8, mesh=small_dragon(40), sky=scenes.procedural_sky(64, 32)),
    "c4": lambda: scenes.config_c4(64, 36, 8, mesh=small_dragon(40)),   # glass, metal, plastic, matte
    "c1": lambda: scenes.config_c1(32, 32, 8),                          # spheres
}
SAMPLERS = {"halton": capi.SAMPLER_HALTON, "sobol": capi.SAMPLER_SOBOL}
_scenes, _values = {}, {}


def scene(kind):
    if kind not in _scenes:
        _scenes[kind] = SCENES[kind]()
    return _scenes[kind]


def with_(rd, spp=None, sampler=None, tiles=None, camera=None):
    if tiles is None and rd.n_tiles:
        tiles = [(rd.tiles[i].x0, rd.tiles[i].y0, rd.tiles[i].x1, rd.tiles[i].y1) for i in range(rd.n_tiles)]
    return scenes.render_desc(rd.camera if camera is None else camera, rd.integrator, rd.spp if spp is None else spp,
                              rd.max_depth, rd.rr_threshold, rd.light_strategy, rd.sampler if sampler is None else sampler,
                              tiles=tiles)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def query_words(hip, rays):
    """pbr_hip_query's records as float32 words [n, 28]: ns = [:, 15:18], uv = [:, 24:26]."""
    import ctypes as C
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
    out = (capi.SurfaceHit * max(1, r.shape[0]))()
    hip._check(hip.lib.pbr_hip_query(hip.ctx, r.shape[0], capi.fptr(r), 0, -1, out), "query")
    assert C.sizeof(capi.SurfaceHit) == 112
    return np.frombuffer(out, dtype=np.float32).reshape(-1, 28)[:r.shape[0]].copy()


def normals(hip):
    return lambda rays: query_words(hip, rays)[:, 15:18]


def aov(hip, rd, first, n, acc=None, image=True, stream=None, sync=True):
    """One render_aov call: (accumulator, image) device tensors; a fresh accumulator is NaN-filled."""
    npx = HipRenderer.n_pixels(rd)
    if acc is None:
        acc = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    img = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV) if image else None
    torch.cuda.synchronize()   # (the fills run on torch's stream, the pass on its own)
    hip.render_aov(rd, first, n, acc.data_ptr(), img.data_ptr() if image else None,
                   stream=None if stream is None else stream.cuda_stream)
    if sync:
        hip.sync()
        torch.cuda.synchronize()
    return acc, img


def values(hip, kind, sampler, n=8):
    """The per-sample expected values of samples 0..n-1 of a SCENES frame, computed once (the scene must be uploaded)."""
    key = (kind, sampler, n)
    if key not in _values:
        s, rd = scene(kind)
        _values[key] = E.sample_values(s, with_(rd, spp=n, sampler=SAMPLERS[sampler]), 0, n, normals(hip))
    return _values[key]


def check(acc, img, want_acc, k, what=""):
    a, i = acc.cpu().numpy(), img.cpu().numpy()
    want_img = E.image(want_acc, k)
    for c, name in enumerate(("albedo.r", "albedo.g", "albedo.b", "hit", "ns.x", "ns.y", "ns.z", "t")):
        assert same(a[:, c], want_acc[:, c]), f"{what}: accumulator channel {name}"
        assert same(i[:, c], want_img[:, c]), f"{what}: image channel {name}"


# ------------------------------------------------------------------ 1. parity with the oracle-built expectation
@pytest.mark.parametrize("spp", [1, 3, 8])
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_parity_with_the_expectation(hip, kind, sampler, spp):
    s, rd = scene(kind)
    hip.upload(s)
    v = values(hip, kind, sampler)
    acc, img = aov(hip, with_(rd, spp=spp, sampler=SAMPLERS[sampler]), 0, spp)
    want = E.accumulate(v[:, :spp])
    assert 0 < want[:, 3].sum() < spp * want.shape[0], "the frame should hold hits and misses"
    check(acc, img, want, spp, f"{kind} {sampler} {spp} spp")


def test_a_pixel_of_two_folding_rounds(hip):
    """260 samples per pixel: the pixel is alone in its workgroup and its sums are carried over two rounds."""
    s, rd = scene("c2")
    hip.upload(s)
    cam = scenes.camera(8, 4, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    rd2 = with_(rd, spp=260, sampler=capi.SAMPLER_HALTON, camera=cam)
    acc, img = aov(hip, rd2, 0, 260)
    want, _ = E.expected(s, rd2, 0, 260, normals(hip))
    check(acc, img, want, 260, "260 spp")


def test_one_pixel_one_sample(hip):
    """A 1×1 frame at 1 sample: one lane of one wave is live."""
    s, rd = scene("c1")
    hip.upload(s)
    cam = scenes.camera(1, 1, (0.0, 0.0, 5.0), (-1.0, 0.0, 0.0), fov=10.0)   # (the whole pixel lies on the first sphere)
    rd2 = with_(rd, spp=1, sampler=capi.SAMPLER_HALTON, camera=cam)
    acc, img = aov(hip, rd2, 0, 1)
    want, _ = E.expected(s, rd2, 0, 1, normals(hip))
    assert want[0, 3] == 1
    check(acc, img, want, 1, "1x1")


# ------------------------------------------------------------------ 2. passes are exact
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_any_cut_into_passes_leaves_the_same_bits(hip, sampler):
    s, rd = scene("c4")
    hip.upload(s)
    rd8 = with_(rd, spp=8, sampler=SAMPLERS[sampler])
    one, one_img = aov(hip, rd8, 0, 8)   # (starts from a NaN-filled accumulator: first_sample = 0 never reads it)
    assert torch.isfinite(one).all() and torch.isfinite(one_img).all()
    for cut in ((2, 3, 3), (1,) * 8):
        acc, img, at, images = None, None, 0, {}
        for n in cut:
            acc, img = aov(hip, rd8, at, n, acc)
            at += n
            images[at] = img.cpu().numpy()
        assert same(acc.cpu().numpy(), one.cpu().numpy()), f"accumulator after {cut}"
        assert same(img.cpu().numpy(), one_img.cpu().numpy()), f"image after {cut}"
        if cut == (2, 3, 3):   # the pass images at k = 2 and k = 5 are those of a fresh single pass of k samples
            for k in (2, 5):
                _, fresh = aov(hip, rd8, 0, k)
                assert same(images[k], fresh.cpu().numpy()), f"pass image at {k} samples"


# ------------------------------------------------------------------ 3. tiles
def test_odd_tiles_equal_the_same_pixels_of_the_frame(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd3 = with_(rd, spp=3, sampler=capi.SAMPLER_HALTON)
    whole, whole_img = aov(hip, rd3, 0, 3)
    tiles = [(11, 5, 16, 8), (40, 30, 47, 32)]   # 5×3 and 7×2, aligned to nothing
    acc, img = aov(hip, with_(rd3, tiles=tiles), 0, 3)
    w = rd.camera.width
    idx = [y * w + x for (x0, y0, x1, y1) in tiles for y in range(y0, y1) for x in range(x0, x1)]
    assert same(acc.cpu().numpy(), whole.cpu().numpy()[idx])
    assert same(img.cpu().numpy(), whole_img.cpu().numpy()[idx])


def test_two_ranks_assemble_to_the_frame(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd3 = with_(rd, spp=3, sampler=capi.SAMPLER_SOBOL)
    _, whole_img = aov(hip, rd3, 0, 3)
    w, h = rd.camera.width, rd.camera.height
    frame = np.zeros((h, w, 8), dtype=np.float32)
    for rank in range(2):
        tiles = tiles_for_rank(w, h, rank, 2)
        _, img = aov(hip, with_(rd3, tiles=tiles), 0, 3)
        part = assemble(w, h, tiles, img.cpu().numpy(), channels=8)
        for (x0, y0, x1, y1) in tiles:
            frame[y0:y1, x0:x1] = part[y0:y1, x0:x1]
    assert same(frame.reshape(-1, 8), whole_img.cpu().numpy())


# ------------------------------------------------------------------ 4. Sobol sample indices above 2^32
@pytest.mark.parametrize("first,n", [(256, 64), (250, 12)], ids=["high_bits_set", "across_the_boundary"])
def test_sobol_wide_indices(hip, first, n):
    """The 4096-wide raster of test_sobol_wide_index_passes at 512 spp: from sample 256 on, the index's
    bits >= 32 are 1.  The pass continues a zero accumulator, so the expectation is the pass's own sum."""
    s, rd = scenes.config_c3(4096, 8, 512, mesh=small_dragon(24))
    rd2 = scenes.render_desc(rd.camera, rd.integrator, 512, 3, rd.rr_threshold, rd.light_strategy, capi.SAMPLER_SOBOL,
                             tiles=[(2040, 2, 2056, 4)])
    hip.upload(s)
    _, idx = E.camera_rays(rd2, first, n)
    assert (idx >= 2 ** 32).any() and ((idx < 2 ** 32).any() == (first < 256))
    zero = torch.zeros((HipRenderer.n_pixels(rd2), 8), dtype=torch.float32, device=DEV)
    acc, img = aov(hip, rd2, first, n, zero)
    want, _ = E.expected(s, rd2, first, n, normals(hip), acc=np.zeros((32, 8), dtype=f32))
    assert want[:, 3].sum() > 0
    check(acc, img, want, first + n, f"samples [{first}, {first + n})")


# ------------------------------------------------------------------ 5. textures
def tex_lookup_np(img, su, sv):
    """tex_lookup in float32 numpy, wrap = repeat: the weights first, then w00·a + w01·b + w10·c + w11·d left to right."""
    h, w = img.shape[:2]
    s, u = su * f32(w) - f32(0.5), sv * f32(h) - f32(0.5)
    s0, u0 = np.floor(s).astype(np.int64), np.floor(u).astype(np.int64)
    ds, du = s - s0.astype(f32), u - u0.astype(f32)
    one = f32(1)
    w00, w01, w10, w11 = (one - ds) * (one - du), (one - ds) * du, ds * (one - du), ds * du
    tx = lambda si, ui: img[ui % h, si % w].astype(f32)
    a, b, c, d = tx(s0, u0), tx(s0, u0 + 1), tx(s0 + 1, u0), tx(s0 + 1, u0 + 1)
    out = w00[:, None] * a + w01[:, None] * b + w10[:, None] * c + w11[:, None] * d
    assert out.dtype == np.float32
    return out


def test_textured_albedo_and_the_instantiation_taken(hip):
    img = (RS.texture_image(16, 8, 3) - f32(0.1)).astype(f32)   # (some texels below 0: the material's clamp shows)
    mapping = (2.0, 1.5, 0.1, -0.2)
    s = scenes.Scene()
    P, I, UV = RS.uv_patch()
    t = s.image_texture(img, wrap=capi.WRAP_REPEAT, mapping=mapping)
    s.textures[t].level0 = 1
    s.mesh(P, I, s.set_texture(s.matte((0.5, 0.5, 0.5)), capi.TEX_KD, t), uv=UV)
    s.point_light((0.0, 4.0, 4.0), (20.0, 20.0, 20.0))
    rd = scenes.render_desc(scenes.camera(40, 24, **RS.CAM_C), capi.INTEGRATOR_PATH, 3, 3)
    hip.upload(s)

    def albedo(rays, hit, prim):
        uv = query_words(hip, rays)[:, 24:26]
        su, sv, du, dv = (f32(m) for m in mapping)
        val = tex_lookup_np(img, su * uv[:, 0] + du, sv * uv[:, 1] + dv)
        return np.maximum(val, f32(0))

    hip.set_profiling(True)
    acc, out = aov(hip, rd, 0, 3)
    prof = hip.get_profile()
    assert "k_aov_tex" in prof and "k_aov" not in prof, sorted(prof)
    want, _ = E.expected(s, rd, 0, 3, normals(hip), albedo=albedo)
    assert want[:, 3].sum() > 0 and np.unique(want[:, 0]).size > 50
    check(acc, out, want, 3, "textured Kd")
    # an untextured scene takes the untextured instantiation
    s2, rd2 = scene("c2")
    hip.upload(s2)
    aov(hip, with_(rd2, spp=1, sampler=capi.SAMPLER_HALTON), 0, 1)
    prof = hip.get_profile()
    hip.set_profiling(False)
    assert "k_aov" in prof and "k_aov_tex" not in prof, sorted(prof)
    assert prof["k_aov"]["launches"] == 1


# ------------------------------------------------------------------ 6. thin lens
def test_the_thin_lens_is_wired(hip):
    """A quad filling the view at the focal distance: every lens sample still hits it.  The camera function
    is the render's own (pinned by the thin-lens render fixtures); this shows the lens dimensions are drawn."""
    kd = (0.25, 0.5, 0.75)
    s = scenes.Scene()
    P, I = vquad(0.0, 30.0)
    s.mesh(P, I, s.matte(kd))
    s.point_light((0.0, 0.0, 2.0), (5.0, 5.0, 5.0))
    pin = scenes.camera(24, 16, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0))
    lens = scenes.camera(24, 16, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0))
    lens.lens_radius, lens.focal_distance = 0.2, 3.0
    hip.upload(s)
    ns = query_words(hip, np.array([[0.1, 0.2, 3.0, 0.0, 0.0, -1.0, np.inf]], dtype=f32))[0, 15:18]
    assert abs(ns[2]) == 1 and ns[0] == 0 and ns[1] == 0
    per_sample = np.zeros((24 * 16, 4, 8), dtype=f32)
    per_sample[:, :, 4:7] = ns
    want_ns = E.image(E.accumulate(per_sample), 4)[:, 4:7]   # (in-order sums from +0: a component of -0 ends as +0)
    got = {}
    for name, cam in (("pinhole", pin), ("lens", lens)):
        for smp in SAMPLERS.values():
            rd = scenes.render_desc(cam, capi.INTEGRATOR_PATH, 4, 3, sampler=smp)
            acc, img = aov(hip, rd, 0, 4)
            a, i = acc.cpu().numpy(), img.cpu().numpy()
            assert np.array_equal(i[:, 3], np.ones(24 * 16, dtype=f32)), "coverage"
            assert same(i[:, 0:3], np.tile(np.asarray(kd, dtype=f32), (24 * 16, 1))), "albedo"   # (4·Kd / 4 is exact)
            assert same(i[:, 4:7], want_ns), "normal"
            assert np.isfinite(i[:, 7]).all() and (i[:, 7] > 0).all()
            got[(name, smp)] = a
    for smp in SAMPLERS.values():
        assert not np.array_equal(got[("pinhole", smp)][:, 7], got[("lens", smp)][:, 7]), "the lens changes no distance"


# ------------------------------------------------------------------ 7. material-less boundaries
def boundary_scene(box):
    s = scenes.Scene()
    P, I = vquad(-2.0, 40.0)
    s.mesh(P, I, s.matte((0.3, 0.6, 0.9)))
    if box:
        Pb, Ib = RS.box((-0.5, -0.5, 0.5), (0.5, 0.5, 1.5))
        s.mesh(Pb, Ib, -1)   # no material: a medium interface
    s.point_light((0.0, 0.0, 2.0), (5.0, 5.0, 5.0))
    return s, scenes.render_desc(scenes.camera(32, 32, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), fov=90.0), capi.INTEGRATOR_PATH, 3, 3)


def test_material_less_faces_are_passed_through(hip):
    """Channels 0-6 on the bits; the distance within 1e-5 relative: two crossings, each moving the origin by at
    most (gamma(7) + 1 ulp)·|p| / cos θ with cos θ >= 0.5, plus three float additions: about 2e-6, fivefold margin."""
    plain, rd = boundary_scene(False)
    hip.upload(plain)
    a0, i0 = (t.cpu().numpy() for t in aov(hip, rd, 0, 3))
    boxed, _ = boundary_scene(True)
    hip.upload(boxed)
    a1, i1 = (t.cpu().numpy() for t in aov(hip, rd, 0, 3))
    assert np.array_equal(a0[:, 3], np.full(32 * 32, 3, dtype=f32))
    assert same(a1[:, :7], a0[:, :7]) and same(i1[:, :7], i0[:, :7])
    assert not np.array_equal(a1[:, 7], a0[:, 7]), "no ray crossed the box"
    rel = float(np.abs(a1[:, 7].astype(np.float64) / a0[:, 7].astype(np.float64) - 1.0).max())
    rel_img = float(np.abs(i1[:, 7].astype(np.float64) / i0[:, 7].astype(np.float64) - 1.0).max())
    assert rel <= 1e-5 and rel_img <= 1e-5, f"distance through the box off by {rel:.3g} (sums), {rel_img:.3g} (image) relative"


def test_the_crossing_bound_fails_the_frame_and_the_context_recovers(hip):
    """1100 nested material-less quads and nothing else: more crossings than the bound of 1024, so the device
    guard fails the call or the following sync; an ordinary render afterwards is correct."""
    s = scenes.Scene()
    zs = np.linspace(-4.0, 2.0, 1100, dtype=np.float32)
    P = np.concatenate([vquad(z, 30.0)[0] for z in zs])
    I = np.concatenate([vquad(0.0, 30.0)[1] + 4 * k for k in range(zs.size)])
    s.mesh(P, I.astype(np.int32), -1)
    s.point_light((0.0, 0.0, 2.0), (5.0, 5.0, 5.0))
    rd = scenes.render_desc(scenes.camera(4, 4, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0)), capi.INTEGRATOR_PATH, 1, 3)
    hip.upload(s)
    acc = torch.zeros((16, 8), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(PbrError, match=r"\(-4\)"):   # PBR_E_UNSUPPORTED
        hip.render_aov(rd, 0, 1, acc.data_ptr())
        hip.sync()
    s1, rd1 = scenes.config_c1(32, 32, 2)
    hip.upload(s1)
    g, g8, _ = hip.render(rd1)
    c, c8, _ = O.render(s1, rd1)
    assert_parity(g, c, g8, c8)


# ------------------------------------------------------------------ 8. a tree too deep for the quad walk
def test_the_binary_walk_scene(hip):
    from test_stack_depth import deep_scene
    s = deep_scene()
    rd = scenes.render_desc(scenes.camera(16, 9, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0)), capi.INTEGRATOR_WHITTED, 3, 3)
    hip.upload(s)
    acc, img = aov(hip, rd, 0, 3)
    want, _ = E.expected(s, rd, 0, 3, normals(hip))
    assert 0 < want[:, 3].sum()
    check(acc, img, want, 3, "47-level chain")


# ------------------------------------------------------------------ 9. bystanders
def test_renders_and_passes_are_unchanged_by_feature_passes(hip):
    s, rd = scene("c2")
    hip.upload(s)
    rd4 = with_(rd, spp=4, sampler=capi.SAMPLER_HALTON)
    want_acc = E.accumulate(values(hip, "c2", "halton")[:, :4])
    c, c8, _ = O.render(s, rd4)
    aov(hip, rd4, 0, 4)
    g, g8, _ = hip.render(rd4)
    assert same(g, c) and np.array_equal(g8, c8), "render after feature passes"
    # a feature pass on a second stream between two progressive passes on the first (the drain rule)
    npx = HipRenderer.n_pixels(rd4)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    pacc = torch.full((npx, 6), NAN, dtype=torch.float32, device=DEV)
    rgb = torch.full((npx, 3), NAN, dtype=torch.float32, device=DEV)
    rgba = torch.zeros((npx, 4), dtype=torch.uint8, device=DEV)
    facc = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    fimg = torch.full((npx, 8), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.render_passes(rd4, 0, 2, pacc.data_ptr(), [None], [None], stream=s1.cuda_stream)
    hip.render_aov(rd4, 0, 4, facc.data_ptr(), fimg.data_ptr(), stream=s2.cuda_stream)
    hip.render_passes(rd4, 2, 2, pacc.data_ptr(), [rgb.data_ptr()], [rgba.data_ptr()], stream=s1.cuda_stream)
    hip.sync()
    torch.cuda.synchronize()
    assert same(rgb.cpu().numpy(), c) and np.array_equal(rgba.cpu().numpy(), c8), "passes around a feature pass"
    check(facc, fimg, want_acc, 4, "feature pass between two passes")


# ------------------------------------------------------------------ 10. the Python layer
def test_progressive_render_with_features(hip):
    s, rd = scene("c4")
    hip.upload(s)
    rd8 = with_(rd, spp=8, sampler=capi.SAMPLER_HALTON)
    one = ProgressiveRender(hip, rd8, features=True)
    rgb1, rgba1 = one.step(8)
    f1 = {k: v.cpu().numpy() for k, v in one.features().items()}
    want_acc = E.accumulate(values(hip, "c4", "halton"))
    want = E.image(want_acc, 8)
    assert same(f1["albedo"], want[:, 0:3]) and same(f1["coverage"], want[:, 3])
    assert same(f1["normal"], want[:, 4:7]) and same(f1["depth"], want[:, 7])
    assert f1["albedo"].shape == (64 * 36, 3) and f1["coverage"].shape == (64 * 36,)
    a = ProgressiveRender(hip, rd8, features=True)
    a.step(2)
    a.step(3)
    st = a.state()
    assert sorted(st) == ["accum", "features", "samples_done"] and st["features"].shape == (64 * 36, 8)
    b = ProgressiveRender(hip, rd8, features=True)
    b.restore(st)
    rgb2, rgba2 = b.step(3)
    f2 = {k: v.cpu().numpy() for k, v in b.features().items()}
    assert same(rgb2.cpu().numpy(), rgb1.cpu().numpy()) and np.array_equal(rgba2.cpu().numpy(), rgba1.cpu().numpy())
    for k in f1:
        assert same(f2[k], f1[k]), k
    assert same(b.state()["features"], want_acc)
    with pytest.raises(ValueError, match="feature accumulator"):
        b.restore({"samples_done": 5, "accum": st["accum"]})
    # features=False: today's state, and no feature pass
    plain = ProgressiveRender(hip, rd8)
    plain.step(2)
    assert sorted(plain.state()) == ["accum", "samples_done"]
    with pytest.raises(ValueError, match="features=False"):
        plain.features()
