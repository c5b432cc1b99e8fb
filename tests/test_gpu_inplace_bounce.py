"""The fused Whitted level 0 tracing whole-wave mirror bounces in place (k_wf_shade's bounce loop).

Where enough lanes of a wave of the fused level-0 shade hold a SpecularReflect continuation and none
has pushed a shadow entry, the wave walks the continuations itself instead of queueing them for the
extend kernel and the next level's shade.  That may not change a bit: every case renders a frame
three ways — the fused wavefront (the new code), the unfused wavefront (none of it) and the
megakernel — over several chunks on two lanes, and compares the float and RGBA8 frames bit for bit.
Profile field 2 of k_wf_shade_l0 counts the rays traced in place; together with the queue pushes
they must be the unfused run's continuations.

The in-place threshold (PBR_WF_INPLACE_MIN) and the number of levels a wave may trace in place
(PBR_WF_INPLACE_ROUNDS) are build switches only, so one setting cannot be compared with another
inside a test run: that comparison is made between builds (tools/ab.sh, which checks every frame
against the first library's)."""
import numpy as np
import pytest
import torch

from pysicalbasedraytracer_amd import HipRenderer, capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def small_dragon(n=48, radius=1.0):
    P, I = scenes.dragon_standin(n=n, radius=radius)
    return P, I, "standin-small"


_sky = []


def sky():
    if not _sky:
        _sky.append(scenes.procedural_sky(128, 64))
    return _sky[0]


_c2 = {}


def c2(width, height, spp, max_depth=5):
    """(scene, a new descriptor) of the C2 builder at a small size; the scene is built once per size."""
    if (width, height) not in _c2:
        _c2[(width, height)] = scenes.config_c2(width, height, 64)
    s, rd = _c2[(width, height)]
    return s, scenes.render_desc(rd.camera, rd.integrator, spp, max_depth)


def render(hip, rd, profile=False, **sched):
    """rd of the uploaded scene under `sched`: (rgb, rgba8, chunk plan, profile or None)."""
    hip.set_schedule(**sched)
    if profile:
        hip.set_profiling(2)
    g, g8, _ = hip.render(rd)
    plan = hip.last_chunks()
    prof = hip.get_profile() if profile else None
    if profile:
        hip.set_profiling(0)
    hip.set_schedule()
    return g, g8, plan, prof


def three_ways(hip, s, rd, chunk_log2, fusable=True):
    """The frame fused, unfused and from the megakernel, compared bit for bit; returns the fused and
    the unfused run's profiles (taken in renders of their own, which must give the same frame)."""
    hip.upload(s)
    mk, mk8, plan, _ = render(hip, rd, kernels=capi.KERNELS_MEGAKERNEL)
    assert plan["n_chunks"] == 0, plan
    assert np.any(mk != 0)
    out = []
    for fuse in (capi.FUSE_ON, capi.FUSE_OFF):
        g, g8, plan, _ = render(hip, rd, chunk_log2=chunk_log2, lanes=2, fuse_camera=fuse)
        if fusable:
            assert plan["n_chunks"] > 1 and plan["lanes"] == 2 and plan["fused_camera"] == (fuse == capi.FUSE_ON), plan
        diff = (bits(g) != bits(mk)).any(axis=1)
        assert not diff.any(), f"fuse {fuse}: {int(diff.sum())} of {len(diff)} float pixels differ from the megakernel's"
        assert np.array_equal(g8, mk8)
        p, p8, _, prof = render(hip, rd, profile=True, chunk_log2=chunk_log2, lanes=2, fuse_camera=fuse)
        assert np.array_equal(bits(p), bits(g)) and np.array_equal(p8, g8)
        out.append(prof)
    return out


def counts(fused, unfused):
    """(rays traced in place, continuations the fused run queued, the unfused run's continuations,
    continuations the fused level 0 queued); the shadow rays must be the same in both runs."""
    def fam(prof, name):   # (a family without a launch, as extend at max_depth 1, is not listed)
        return prof.get(name, {"units": 0, "counts": [0] * 8})

    l0 = fused["k_wf_shade_l0"]
    inplace = l0["counts"][2]
    queued = l0["counts"][4] + fam(fused, "k_wf_shade")["counts"][4]
    total = unfused["k_wf_shade"]["counts"][4]
    print(f"continuations {total}: in place {inplace} ({inplace / max(1, total):.3f}), queued {queued}")
    assert inplace + queued == total
    assert fam(fused, "k_wf_extend")["units"] == queued and fam(unfused, "k_wf_extend")["units"] == total
    assert fused["k_wf_shadow"]["units"] == unfused["k_wf_shadow"]["units"]
    assert "k_wf_shade_l0" not in unfused and unfused["k_wf_shade"]["counts"][2] == 0
    return inplace, queued, total, l0["counts"][4]


@pytest.mark.parametrize("spp,chunk_log2", [(64, 16), (16, 14)])
def test_c2_shape(hip, spp, chunk_log2):
    """The benchmarked scene's shape: a mirror floor over most of the frame.  At 64 spp a wave is one
    pixel's samples (the pixel table), at 16 spp it spans four pixels."""
    s, rd = c2(96, 54, spp)
    fused, unfused = three_ways(hip, s, rd, chunk_log2)
    inplace, _, _, _ = counts(fused, unfused)
    assert inplace > 0


@pytest.mark.parametrize("width,spp", [(96, 20), (95, 20)])
def test_ragged_waves(hip, width, spp):
    """An spp that does not divide 64 (a wave's pixels start anywhere in it), and with the odd width a
    sample count that is no multiple of 64: the last wave of the last chunk has inactive lanes."""
    s, rd = c2(width, 54, spp)
    assert (width * 54 * spp % 64 != 0) == (width == 95)
    fused, unfused = three_ways(hip, s, rd, 14)
    inplace, _, _, _ = counts(fused, unfused)
    assert inplace > 0


@pytest.mark.parametrize("max_depth", [1, 2, 5])
def test_depth_limits_c2(hip, max_depth):
    """max_depth 1: no continuation at all (the loop never goes round); 2: one in-place trip that may
    not continue; 5: C2's own."""
    s, rd = c2(96, 54, 64, max_depth)
    fused, unfused = three_ways(hip, s, rd, 16)
    inplace, queued, total, _ = counts(fused, unfused)
    if max_depth == 1:
        assert inplace == queued == total == 0
    else:
        assert inplace > 0


def mirror_box(width, height, spp, max_depth):
    """A matte body between a mirror floor and a mirror ceiling facing each other, under the SkyBox.
    The plates are 2.3 apart and reach 60 from the centre: a ray that leaves the camera more than 30
    degrees below the horizon (the lower rows: the camera looks 16 degrees down with a 90-degree
    field of view) moves less than 4 along the plates per bounce, so it is still between them after
    15 bounces unless it meets the body."""
    s = scenes.Scene()
    green = s.matte((0.0, 1.0, 0.0))
    mirror = s.mirror((0.9, 0.9, 0.9))
    P, I = scenes.dragon_standin(n=32, radius=0.45)
    s.mesh(P, I, green)
    Pf, If = scenes.quad(-1.0, 60.0)
    s.mesh(Pf, If, mirror)
    Pc, Ic = scenes.quad(1.3, 60.0, flip=True)
    s.mesh(Pc, Ic, mirror)
    s.skybox(sky(), world_radius=60.0)
    cam = scenes.camera(width, height, (0.0, 0.2, 2.4), (0.0, -0.5, 0.0))
    return s, scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, spp, max_depth)


def test_depth_cap_between_mirrors(hip):
    """Two facing mirrors at max_depth 16, the wavefront schedule's deepest.  A chain runs in place for
    PBR_WF_INPLACE_ROUNDS levels (2 as shipped; a build with 16 reaches the level cap inside the
    loop, which only a comparison between builds can show) and goes on through the queue, so a sample's
    levels are shaded partly in place and partly queued, up to the cap.  The deepest level must hold
    rays (the unfused continuations at depth 16 minus those at depth 15), so the cap is exercised."""
    s, rd = mirror_box(64, 36, 64, 16)
    fused, unfused = three_ways(hip, s, rd, 16)
    inplace, _, total, _ = counts(fused, unfused)
    assert inplace > 0
    _, rd15 = mirror_box(64, 36, 64, 15)
    *_, prof15 = render(hip, rd15, profile=True, chunk_log2=16, lanes=2, fuse_camera=capi.FUSE_OFF)
    deepest = total - prof15["k_wf_shade"]["counts"][4]
    print(f"rays at the deepest level: {deepest}")
    assert deepest > 0


def test_mixed_waves(hip):
    """A mirror quad turned 37 degrees on a matte floor, covering part of the frame with its edges
    crossing pixels diagonally: waves wholly on the mirror go round, waves on an edge and waves that
    see the body reflected push to the queue — both in one launch."""
    s = scenes.Scene()
    green = s.matte((0.0, 1.0, 0.0))
    grey = s.matte((0.6, 0.6, 0.6))
    mirror = s.mirror((1.0, 1.0, 1.0))
    P, I, _ = small_dragon()
    s.mesh(P, I, green)
    Pf, If = scenes.quad(-1.13, 40.0)
    s.mesh(Pf, If, grey)
    Pm, Im = scenes.quad(-1.12, 1.6, z0=0.6)
    s.mesh(Pm, Im, mirror, xform=scenes.rotate_y(37.0))   # (degrees)
    s.skybox(sky(), world_radius=60.0)
    cam = scenes.camera(96, 54, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    rd = scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 64, 5)
    fused, unfused = three_ways(hip, s, rd, 15)
    inplace, _, _, queued0 = counts(fused, unfused)
    assert inplace > 0 and queued0 > 0


def lit_scene(light):
    """The C2 layout without the SkyBox: the non-SkyBox level-0 instantiations, whose in-place levels
    push shadow entries with a real pdf."""
    s = scenes.Scene()
    green = s.matte((0.0, 1.0, 0.0))
    mirror = s.mirror((1.0, 1.0, 1.0))
    P, I, _ = small_dragon()
    s.mesh(P, I, green)
    Pf, If = scenes.quad(-1.12, 40.0)
    s.mesh(Pf, If, mirror)
    if light == "point":
        s.point_light((1.0, 3.0, 2.0), (20.0, 18.0, 16.0))
    else:   # one triangle: one DiffuseAreaLight
        white = s.matte((0.8, 0.8, 0.8))
        Pl = np.array([[-1.5, 2.6, 1.0], [1.5, 2.6, 1.0], [0.0, 2.6, -1.5]], dtype=np.float32)
        s.area_light_mesh(Pl, np.array([[0, 1, 2]], dtype=np.int32), (9.0, 9.0, 9.0), white, two_sided=True)
    cam = scenes.camera(96, 54, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    return s, scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 64, 5)


@pytest.mark.parametrize("light", ["point", "area"])
def test_one_light(hip, light):
    s, rd = lit_scene(light)
    assert len(s.lights) == 1
    fused, unfused = three_ways(hip, s, rd, 16)
    inplace, _, _, _ = counts(fused, unfused)
    assert inplace > 0
    assert fused["k_wf_shadow"]["units"] > 0


def test_specular_glass(hip):
    """A specular glass sphere (urough = vrough = 0) beside the body: the simple-lobe instantiation."""
    s = scenes.Scene()
    green = s.matte((0.0, 1.0, 0.0))
    mirror = s.mirror((1.0, 1.0, 1.0))
    glass = s.glass(urough=0.0, vrough=0.0)
    P, I = scenes.dragon_standin(n=48, radius=0.7)
    s.mesh(P, I, green)
    s.sphere((1.3, -0.5, 0.4), 0.6, glass)
    Pf, If = scenes.quad(-1.12, 40.0)
    s.mesh(Pf, If, mirror)
    s.skybox(sky(), world_radius=60.0)
    cam = scenes.camera(96, 54, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    rd = scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 64, 5)
    fused, unfused = three_ways(hip, s, rd, 16)
    inplace, _, _, _ = counts(fused, unfused)
    assert inplace > 0


def test_material_less_primitive(hip):
    """One primitive without a material (Whitted's pass-through branch, which stays on the queue):
    whichever schedule the library picks for such a scene, the three frames are the same."""
    s = scenes.Scene()
    green = s.matte((0.0, 1.0, 0.0))
    mirror = s.mirror((1.0, 1.0, 1.0))
    P, I, _ = small_dragon()
    s.mesh(P, I, green)
    Pp, Ip = scenes.quad(-0.4, 0.8, x0=1.2, z0=0.8)
    s.mesh(Pp, Ip, -1)
    Pf, If = scenes.quad(-1.12, 40.0)
    s.mesh(Pf, If, mirror)
    s.skybox(sky(), world_radius=60.0)
    cam = scenes.camera(96, 54, (0.0, 0.55, 2.6), (0.0, -0.25, 0.0))
    rd = scenes.render_desc(cam, capi.INTEGRATOR_WHITTED, 64, 5)
    hip.upload(s)
    mk, mk8, _, _ = render(hip, rd, kernels=capi.KERNELS_MEGAKERNEL)
    assert np.any(mk != 0)
    for fuse in (capi.FUSE_ON, capi.FUSE_OFF):
        g, g8, _, _ = render(hip, rd, chunk_log2=16, lanes=2, fuse_camera=fuse)
        assert np.array_equal(bits(g), bits(mk)) and np.array_equal(g8, mk8)


def test_progressive_pass_pair(hip):
    """Two passes of 64 samples over a 128-spp descriptor (the PASS instantiation, the second with
    passFirst = 64), fused and unfused, end in the megakernel's 128-spp frame."""
    s, rd = c2(96, 54, 128)
    hip.upload(s)
    mk, mk8, _, _ = render(hip, rd, kernels=capi.KERNELS_MEGAKERNEL)
    npx = 96 * 54
    for fuse in (capi.FUSE_ON, capi.FUSE_OFF):
        hip.set_schedule(chunk_log2=16, lanes=2, fuse_camera=fuse)
        acc = torch.full((npx, 6), float("nan"), dtype=torch.float32, device=DEV)   # the first pass must not read it
        rgbs = [torch.full((npx, 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
        rgbas = [torch.zeros((npx, 4), dtype=torch.uint8, device=DEV) for _ in range(2)]
        torch.cuda.synchronize()
        hip.render_passes(rd, 0, 64, acc.data_ptr(), [t.data_ptr() for t in rgbs], [t.data_ptr() for t in rgbas])
        plan = hip.last_chunks()
        hip.sync()
        torch.cuda.synchronize()
        hip.set_schedule()
        assert plan["fused_camera"] == (fuse == capi.FUSE_ON) and plan["n_chunks"] >= 2, plan
        assert np.array_equal(bits(rgbs[1].cpu().numpy()), bits(mk)) and np.array_equal(rgbas[1].cpu().numpy(), mk8)
        assert (bits(rgbs[0].cpu().numpy()) != bits(mk)).any()   # (64 samples are another image)
