"""pbr_hip_temporal without a GPU: the exports, the struct, every refusal of the Python wrappers before a
device call, pbr_hip_camera_matrices against the oracle's camera rays, and pbr_hip_temporal_host — the
device's per-pixel function compiled for the CPU — against the numpy restatement of the rule
(temporal_expected.py), on the bits.  The one statistical test says that it is one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib
import temporal_expected as TE
from pysicalbasedraytracer_amd import HipRenderer, TemporalRender, capi, scenes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbr_hip.h")
INF, NAN = float("inf"), float("nan")
f32 = np.float32
SHAPES = ((64, 36), (37, 23), (8, 5), (1, 1))


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
    """A renderer without a context: temporal_host needs none."""
    return renderer_without_device(capi.load_library())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_host(kw, what=""):
    """pbr_hip_temporal_host against the restatement on the bits: sums, counts and motion.  Returns the
    restatement's (accum_out, counts_out, motion, took)."""
    want = TE.temporal(**kw)
    got = host().temporal_host(**kw)
    assert same(got[0], want[0]), f"{what}: sums differ at {int((bits(got[0]) != bits(want[0])).any(axis=1).sum())} pixels"
    assert np.array_equal(got[1], want[1]), f"{what}: counts differ at {int((got[1] != want[1]).sum())} pixels"
    assert same(got[2], want[2]), f"{what}: motion differs at {int((bits(got[2]) != bits(want[2])).any(axis=1).sum())} pixels"
    return want


# ------------------------------------------------------------------ 1. symbols, struct, refusals
def test_the_symbols_exist_and_null_arguments_are_rejected():
    lib = capi.load_library()
    I = np.eye(4, dtype=f32)
    p = capi.Temporal(4, 2, 32, 1, 0.05, 0.1)
    p.cur_raster_to_world[:] = p.prev_world_to_raster[:] = I.reshape(-1).tolist()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    cnt = (C.c_int32 * 8)()
    c = C.addressof(cnt)
    out, cout = (C.c_float * 64)(), (C.c_int32 * 8)()
    o, co = C.addressof(out), C.addressof(cout)
    assert lib.pbr_hip_temporal(None, C.byref(p), 4, None, a, a, c, a, a, o, co, None, None, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_temporal_host(C.byref(p), 4, None, a, a, c, a, a, o, co, None) == capi.PBR_OK
    assert lib.pbr_hip_temporal_host(None, 4, None, a, a, c, a, a, o, co, None) == capi.PBR_E_INVALID
    for hole in range(2, 10):   # each required buffer in turn (counts_cur, argument 2, and motion_out may be NULL)
        args = [C.byref(p), 4, None, a, a, c, a, a, o, co, None]
        if hole == 2:
            continue
        args[hole] = None
        assert lib.pbr_hip_temporal_host(*args) == capi.PBR_E_INVALID, hole
    # an output that is one of the history buffers
    assert lib.pbr_hip_temporal_host(C.byref(p), 4, None, a, a, c, o, a, o, co, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_temporal_host(C.byref(p), 4, None, a, a, co, a, a, o, co, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_temporal_host(C.byref(p), 4, None, a, a, c, a, o, o, co, o) == capi.PBR_E_INVALID
    # ... and in place over the current buffers is fine
    assert lib.pbr_hip_temporal_host(C.byref(p), 4, co, o, a, c, a, a, o, co, None) == capi.PBR_OK
    cam = TE.camera(8, 4)
    m = (C.c_float * 16)()
    e = (C.c_float * 3)()
    assert lib.pbr_hip_camera_matrices(C.byref(cam), m, m, e) == capi.PBR_OK
    assert lib.pbr_hip_camera_matrices(None, m, m, e) == capi.PBR_E_INVALID
    assert lib.pbr_hip_camera_matrices(C.byref(cam), None, m, e) == capi.PBR_E_INVALID
    assert lib.pbr_hip_camera_matrices(C.byref(cam), m, None, e) == capi.PBR_E_INVALID
    assert lib.pbr_hip_camera_matrices(C.byref(cam), m, m, None) == capi.PBR_E_INVALID
    cam.width = 0
    assert lib.pbr_hip_camera_matrices(C.byref(cam), m, m, e) == capi.PBR_E_INVALID
    with pytest.raises(ValueError):
        capi.camera_matrices(cam)


def test_the_struct_matches_the_header():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct pbr_temporal \{(.*?)\} pbr_temporal;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        base = {"int": C.c_int, "float": C.c_float}[ctype]
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            fields.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    mine = [(n, t) for n, t in capi.Temporal._fields_]
    assert [n for n, _ in fields] == [n for n, _ in mine]
    assert [C.sizeof(t) for _, t in fields] == [C.sizeof(t) for _, t in mine]
    offsets, off = [], 0
    for _, t in fields:   # (4-byte members throughout: no padding)
        offsets.append(off)
        off += C.sizeof(t)
    assert [getattr(capi.Temporal, n).offset for n, _ in mine] == offsets
    assert C.sizeof(capi.Temporal) == off == 4 * (6 + 16 + 3 + 16 + 3)


MATS = (np.eye(4, dtype=f32), np.eye(4, dtype=f32), np.zeros(3, f32))
GOOD = dict(width=16, height=8, samples=4, accum_cur_ptr=0x1000, aov_cur_ptr=0x2000, counts_prev_ptr=0x3000,
            accum_prev_ptr=0x4000, aov_prev_ptr=0x5000, accum_out_ptr=0x6000, counts_out_ptr=0x7000, cur=MATS, prev=MATS)


def with_nan(which):
    m = [x.copy() for x in MATS]
    m[which].reshape(-1)[1] = NAN
    return tuple(m)


@pytest.mark.parametrize("change", [
    dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 16, height=1 << 15),
    dict(max_history=0), dict(max_history=(1 << 20) + 1), dict(max_history=-1),
    dict(tol_z=-1e-3), dict(tol_z=NAN), dict(tol_n=-1.0), dict(tol_n=NAN),
    dict(samples=0), dict(samples=-2),
    dict(cur=with_nan(0)), dict(cur=with_nan(2)), dict(prev=with_nan(1)), dict(prev=with_nan(2)),
    dict(accum_cur_ptr=0), dict(aov_cur_ptr=None), dict(counts_prev_ptr=0), dict(accum_prev_ptr=None), dict(aov_prev_ptr=0),
    dict(accum_out_ptr=0), dict(counts_out_ptr=None),
    dict(accum_out_ptr=0x4000), dict(counts_out_ptr=0x3000), dict(motion_ptr=0x5000), dict(rgb_ptr=0x4000), dict(rgba_ptr=0x3000),
], ids=lambda c: ",".join(f"{k}={'nan-planted' if isinstance(v, tuple) else v}" for k, v in c.items()))
def test_the_wrapper_refuses_bad_arguments_before_any_device_call(change):
    r = renderer_without_device()
    with pytest.raises(ValueError):
        r.temporal(**{**GOOD, **change})


def test_the_wrapper_passes_good_arguments_on():
    """... so the refusals above are the arguments', not the stand-in's: a good call reaches the library
    (samples is not read when per-pixel counts are given; in place over the current buffers; a NaN in a
    matrix the call does not read)."""
    r = renderer_without_device()
    for change in (dict(), dict(samples=0, counts_cur_ptr=0x8000), dict(accum_out_ptr=0x1000),
                   dict(counts_cur_ptr=0x8000, counts_out_ptr=0x8000), dict(max_history=1), dict(max_history=1 << 20),
                   dict(tol_z=0.0, tol_n=0.0), dict(tol_z=INF), dict(cur=with_nan(1)), dict(prev=with_nan(0)),
                   dict(motion_ptr=0x9000, rgb_ptr=0xa000, rgba_ptr=0xb000)):
        with pytest.raises(AssertionError, match="pbr_hip_temporal was called"):
            r.temporal(**{**GOOD, **change})


def test_the_host_wrapper_refuses_bad_arguments_before_any_library_call():
    r = renderer_without_device()
    good = TE.call_args(TE.synthetic_pair(8, 5, 4, "identity"))
    for change in (dict(width=0), dict(max_history=0), dict(tol_z=NAN), dict(tol_n=-1.0), dict(samples=0), dict(cur=with_nan(0)),
                   dict(prev=with_nan(2)), dict(accum_cur=None), dict(aov_prev=None), dict(counts_prev=None),
                   dict(accum_cur=np.zeros((7, 6), f32)), dict(counts_prev=np.zeros(3, np.int32)),
                   dict(counts_cur=np.zeros(41, np.int32))):
        with pytest.raises(ValueError):
            r.temporal_host(**{**good, **change})
    with pytest.raises(AssertionError, match="pbr_hip_temporal_host was called"):
        r.temporal_host(**good)


def test_temporal_render_refuses():
    r = renderer_without_device()

    def desc(spp, sampler=capi.SAMPLER_HALTON, **kw):
        cam = scenes.camera(16, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
        return scenes.render_desc(cam, capi.INTEGRATOR_PATH, spp, 3, 1.0, capi.LIGHTS_UNIFORM, sampler, **kw)

    TemporalRender(r, desc(64), 4)              # 4 x 16 = 64 fits
    TemporalRender(r, desc(33, capi.SAMPLER_SOBOL), 4)   # Sobol rounds 33 up to 64, as passes do
    for bad in (lambda: TemporalRender(r, desc(63), 4), lambda: TemporalRender(r, desc(32, capi.SAMPLER_SOBOL), 4),
                lambda: TemporalRender(r, desc(64), 0), lambda: TemporalRender(r, desc(64), 4, cycle=0),
                lambda: TemporalRender(r, desc(64), 4, max_history=0), lambda: TemporalRender(r, desc(64), 4, tol_z=NAN),
                lambda: TemporalRender(r, desc(64), 4, tol_n=-1.0), lambda: TemporalRender(r, desc(64, tiles=[(0, 0, 8, 8)]), 4)):
        with pytest.raises(ValueError):
            bad()
    t = TemporalRender(r, desc(64), 4)
    with pytest.raises(ValueError, match="camera"):
        t.frame(scenes.camera(8, 8, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0)))
    with pytest.raises(ValueError, match="no frame yet"):
        t.denoise()
    with pytest.raises(ValueError, match="no frame yet"):
        t.history()


# ------------------------------------------------------------------ 2. the matrices
def cameras(w, h):
    """A use_look_at camera, and the same camera handed over as matrices with a RasterToCamera of its own
    (fov 60, its own screen window), the way the reference binding hands a PerspectiveCamera over."""
    eye, at, up = np.array((0.3, 0.5, 2.0)), np.array((0.0, 0.0, -4.0)), np.array((0.0, 1.0, 0.0))
    look = scenes.camera(w, h, tuple(eye), tuple(at), tuple(up), fov=70.0)
    unit = lambda v: v / np.linalg.norm(v)
    fwd = unit(at - eye)
    right = unit(np.cross(unit(up), fwd))
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, eye
    n, f, c = 1e-2, 1000.0, 1.0 / np.tan(np.radians(60.0) / 2)
    persp = np.array([[c, 0, 0, 0], [0, c, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1, 0]])
    x0, x1, y0, y1 = -1.2, 1.5, -0.8, 0.9   # a screen window of its own
    s2r = np.diag([w, h, 1, 1.0]) @ np.diag([1 / (x1 - x0), 1 / (y0 - y1), 1, 1.0])
    s2r = s2r @ np.array([[1, 0, 0, -x0], [0, 1, 0, -y1], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    r2c = np.linalg.inv(persp) @ np.linalg.inv(s2r)
    xf = lambda m: scenes._xf((m.astype(f32), np.linalg.inv(m).astype(f32)))
    given = capi.CameraDesc(width=w, height=h, use_look_at=0, fov=90.0, lens_radius=0.0, focal_distance=0.0, medium=-1,
                            use_raster_to_camera=1, camera_to_world=xf(c2w), raster_to_camera=xf(r2c))
    return {"use_look_at": look, "use_raster_to_camera": given}


def pinhole_rays(mats, w, h):
    """Unit directions through the pixel centres from raster_to_world and eye, in float64."""
    r2w, eye = mats[0].astype(np.float64), mats[2].astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    pr = np.stack([xs + 0.5, ys + 0.5, np.zeros((h, w)), np.ones((h, w))], -1) @ r2w.T
    d = pr[..., :3] / pr[..., 3:4] - eye
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


@pytest.mark.parametrize("kind", ["use_look_at", "use_raster_to_camera"])
def test_the_matrices_give_the_oracles_camera_rays(kind):
    w, h = 64, 36
    cam = cameras(w, h)[kind]
    mats = capi.camera_matrices(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    pfilm = np.stack([xs + 0.5, ys + 0.5], -1).reshape(-1, 2).astype(f32)
    rays = oracle_lib.camera_rays(cam, pfilm)
    err_o = float(np.abs(rays[:, 0:3] - mats[2]).max())
    err_d = float(np.abs(pinhole_rays(mats, w, h) - rays[:, 3:6]).max())
    print(f"{kind}: origin error {err_o:.3g}, direction error {err_d:.3g}")
    assert err_o <= 1e-5 and err_d <= 1e-5


@pytest.mark.parametrize("kind", ["use_look_at", "use_raster_to_camera"])
def test_identity_motion_reprojects_a_pixel_onto_itself(kind):
    w, h = 64, 36
    cam = cameras(w, h)[kind]
    accum, aov, _, mats = TE.synthetic_frame(cam, 4, seed=5)
    cnt = np.full(w * h, 4, np.int32)
    out, counts, motion, took = check_host(dict(width=w, height=h, samples=4, accum_cur=accum, aov_cur=aov, counts_prev=cnt,
                                                accum_prev=accum, aov_prev=aov, cur=mats, prev=mats), kind)
    hit = aov[:, 3] > 0
    assert hit.sum() > w * h // 2
    worst = float(np.abs(motion[hit]).max())
    print(f"{kind}: identity motion reprojects to within {worst:.3g} px")
    assert worst <= 1e-3
    assert took[hit].all() and not took[~hit].any()
    assert np.array_equal(counts, np.where(hit, 8, 4))


# ------------------------------------------------------------------ 3. the host twin against the restatement
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("motion", TE.MOTIONS)
def test_the_host_twin_equals_the_restatement(motion, demodulate):
    for (w, h) in SHAPES:
        pair = TE.synthetic_pair(w, h, 4, motion)
        check_host(TE.call_args(pair, demodulate=demodulate), f"{motion} {w}x{h}")


def test_the_inputs_exercise_the_rule():
    """Conditions on the inputs, on the restatement alone, so that the comparisons above cannot pass
    vacuously: a sub-pixel pan and both dollies give history to at least half the hit pixels at 64x36 (the
    prototype: over 0.9); a pan out of the frame and a camera turned round give none, and then the output is
    the input bit for bit."""
    for motion in TE.MOTIONS:
        pair = TE.synthetic_pair(64, 36, 4, motion)
        out, counts, mot, took = TE.temporal(**TE.call_args(pair))
        hit = pair["aov_cur"][:, 3] > 0
        share = took.sum() / hit.sum()
        print(f"{motion}: {int(hit.sum())} hit pixels, {share:.3f} take history")
        assert 0 < hit.sum() < hit.size, "the frame should hold hits and misses"
        if motion in ("subpixel_pan", "dolly_in", "dolly_out", "identity"):
            assert share >= 0.5
            assert not same(out, pair["accum_cur"])
        if motion in ("pan_out", "turned_round"):
            assert share == 0
            assert same(out, pair["accum_cur"]) and np.array_equal(counts, np.full(64 * 36, 4, np.int32))
        if motion == "turned_round":
            assert not mot.any(), "behind the previous camera: no projection, no motion"
        if motion == "subpixel_pan":
            assert 0 < np.abs(mot[took]).max() < 1, "a sub-pixel pan"


@pytest.mark.parametrize("motion", ["subpixel_pan", "dolly_in", "roll90"])
def test_per_pixel_counts_with_zero_and_one(motion):
    for (w, h) in ((64, 36), (37, 23)):
        pair = TE.synthetic_pair(w, h, 4, motion)
        rng = np.random.default_rng(w)
        cc = rng.integers(0, 9, w * h).astype(np.int32)
        cp = rng.integers(0, 40, w * h).astype(np.int32)
        cp[rng.integers(0, w * h, w * h // 8)] = 1
        assert (cc == 0).any() and (cc == 1).any() and (cp == 0).any() and (cp == 1).any()
        out, counts, _, took = check_host(TE.call_args(pair, counts_cur=cc, counts_prev=cp, samples=0), f"{motion} {w}x{h}")
        assert took.any() and (counts[took] > cc[took]).all() and np.array_equal(counts[~took], cc[~took])
        assert (counts[took] - cc[took]).max() <= 32, "the default max_history caps the history"


@pytest.mark.parametrize("max_history", [1, 1 << 20])
def test_the_max_history_extremes(max_history):
    pair = TE.synthetic_pair(37, 23, 4, "dolly_out")
    cp = np.full(37 * 23, (1 << 20) + 5, np.int32)
    out, counts, _, took = check_host(TE.call_args(pair, counts_prev=cp, max_history=max_history), f"max_history {max_history}")
    assert took.any() and (counts[took] == 4 + max_history).all()


def test_a_nan_and_an_infinity_in_the_history_enter_no_pixel():
    for demod in (False, True):
        pair = TE.synthetic_pair(37, 23, 4, "subpixel_pan")
        ap = pair["accum_prev"].copy()
        hitp = np.flatnonzero(pair["aov_prev"][:, 3] > 0)
        p_nan, p_inf = int(hitp[len(hitp) // 3]), int(hitp[2 * len(hitp) // 3])
        ap[p_nan, 1] = NAN
        ap[p_inf, 4] = INF
        clean = TE.temporal(**TE.call_args(pair, demodulate=demod))
        out, counts, _, took = check_host(TE.call_args(pair, accum_prev=ap, demodulate=demod), "planted history")
        assert np.isfinite(out).all(), "no output pixel may be non-finite: the planted values are in the history"
        assert not same(out, clean[0]), "the planted taps were in use: dropping them changes the neighbours"


def test_a_nan_current_pixel_stays_on_itself():
    pair = TE.synthetic_pair(37, 23, 4, "subpixel_pan")
    ac = pair["accum_cur"].copy()
    p = int(np.flatnonzero(pair["aov_cur"][:, 3] > 0)[100])
    ac[p, 2] = NAN
    out, _, _, _ = check_host(TE.call_args(pair, accum_cur=ac), "NaN current pixel")
    bad = ~np.isfinite(out).all(axis=1)
    assert bad.sum() == 1 and bad[p]


def test_in_place_over_the_current_buffers():
    """accum_out = accum_cur and counts_out = counts_cur: the bits of the out-of-place call."""
    lib = capi.load_library()
    pair = TE.synthetic_pair(37, 23, 4, "dolly_in")
    kw = TE.call_args(pair)
    want = TE.temporal(**kw)
    p = HipRenderer._check_temporal("test", 37, 23, 4, True, 32, 0.05, 0.1, pair["cur"], pair["prev"])
    p.demodulate = 1
    acc = pair["accum_cur"].copy()
    cnt = np.full(37 * 23, 4, np.int32)
    ptr = lambda a: a.ctypes.data
    rc = lib.pbr_hip_temporal_host(C.byref(p), 0, ptr(cnt), ptr(acc), ptr(pair["aov_cur"]), ptr(pair["counts_prev"]),
                                   ptr(pair["accum_prev"]), ptr(pair["aov_prev"]), ptr(acc), ptr(cnt), None)
    assert rc == capi.PBR_OK
    assert same(acc, want[0]) and np.array_equal(cnt, want[1])


# ------------------------------------------------------------------ 4. a history over several frames
def test_the_history_saturates_at_max_history():
    """Eight identity frames of k = 4 with max_history 8: counts of 4, 8, 12, 12, ... on the hit pixels (the
    history length is k + min(previous, max_history): a capped moving average), 4 on the others."""
    w, h, k = 37, 23, 4
    cam = TE.camera(w, h)
    hist = None
    seen = []
    for f in range(8):
        accum, aov, _, mats = TE.synthetic_frame(cam, k, seed=20 + f)
        if hist is None:
            hist = (accum, np.full(w * h, k, np.int32), aov)
        else:
            out, counts, _, _ = check_host(dict(width=w, height=h, samples=k, accum_cur=accum, aov_cur=aov, counts_prev=hist[1],
                                                accum_prev=hist[0], aov_prev=hist[2], cur=mats, prev=mats, max_history=8), f"frame {f}")
            hist = (out, counts, aov)
        hit = aov[:, 3] > 0
        assert (hist[1][~hit] == k).all()
        assert len(set(hist[1][hit].tolist())) == 1
        seen.append(int(hist[1][hit][0]))
    assert seen == [4, 8, 12, 12, 12, 12, 12, 12]


def test_a_panning_history_is_closer_to_the_truth():
    """Statistical, not on the bits: eight frames of 4 samples at 64x36, the camera panning 0.2 units per frame,
    max_history 32.  On the pixels of the last frame that took history, the squared error against the truth
    (float64 sums) of the merged frame must be strictly below the single frame's with demodulate; both ratios
    are printed (without demodulation the bilinear resampling blurs the floor's texture into the history)."""
    w, h, k = 64, 36, 4
    ratios = {}
    for demod in (True, False):
        hist = prev = None
        for f in range(8):
            cam = TE.camera(w, h, eye=(0.2 * f, 0.5, 2.0), look=(0.2 * f, 0.0, -4.0))
            accum, aov, truth, mats = TE.synthetic_frame(cam, k, seed=40 + f)
            if hist is None:
                hist, took = (accum, np.full(w * h, k, np.int32), aov), None
            else:
                out, counts, _, took = TE.temporal(w, h, k, accum, aov, hist[1], hist[0], hist[2], mats, prev, max_history=32,
                                                   demodulate=demod)
                hist = (out, counts, aov)
            prev = mats
        assert took.sum() >= 0.5 * (aov[:, 3] > 0).sum()
        t = truth.astype(np.float64)[took]
        e_one = float(((accum[took, :3].astype(np.float64) / k - t) ** 2).sum())
        e_hist = float(((TE.image(hist[0], hist[1]).astype(np.float64)[took] - t) ** 2).sum())
        ratios[demod] = e_hist / e_one
        print(f"demodulate {demod}: squared error on {int(took.sum())} history pixels: single frame {e_one:.6g}, "
              f"merged {e_hist:.6g}, ratio {ratios[demod]:.4f}")
    assert ratios[True] < 1
