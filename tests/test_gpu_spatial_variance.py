"""pbr_hip_denoise_sv on the device: the denoiser with the spatial variance estimate between prepare and level 0.

Every comparison is on the bits (uint32 views) against spatial_variance_expected.py, the numpy restatement of
the rule, over inputs copied back from the device; rgba against the restated film transform of the device's
own rgb.  The one statistical test (quality on a render) says so."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoise_expected as DE
import spatial_variance_expected as SE
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, TemporalRender, capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
NAN, INF = float("nan"), float("inf")
W, H = 64, 36
SHAPES = ((1, 1), (7, 3), (33, 9), (70, 21))   # one pixel; smaller than the window; one past a tile both ways; several tiles
COUNT_SET = (0, 1, 2, 3, 4, 9)


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def small_dragon(n=40):
    P, I = scenes.dragon_standin(n=n)
    return P, I, "standin-small"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def path_desc(rd, spp, cam=None):
    return scenes.render_desc(cam if cam is not None else rd.camera, capi.INTEGRATOR_PATH, spp, rd.max_depth, rd.rr_threshold,
                              rd.light_strategy, capi.SAMPLER_HALTON)


_scene = {}


def scene(hip):
    """The small C4-style Path scene of tests/test_gpu_denoise.py (glass, metal, plastic, matte under an area
    light) at 64x36, uploaded once: (scene, descriptor)."""
    if not _scene:
        s, rd = scenes.config_c4(W, H, 8, mesh=small_dragon(40))
        hip.upload(s)
        _scene.update(s=s, rd=rd)
    return _scene["s"], _scene["rd"]


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


def run(hip, w, h, samples, acc, aov, counts=None, stream=None, **params):
    """One denoise call over device tensors (numpy inputs are uploaded); NaN / zero-filled outputs back as
    numpy: (rgb [n, 3], rgba [n, 4], var [n])."""
    dev = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    acc, aov = dev(acc, np.float32), dev(aov, np.float32)
    cnt = None if counts is None else dev(counts, np.int32)
    n = w * h
    rgb = torch.full((n, 3), NAN, dtype=torch.float32, device=DEV)
    rgba = torch.zeros((n, 4), dtype=torch.uint8, device=DEV)
    var = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()   # (uploads and fills run on torch's stream, the call on its own)
    hip.denoise(w, h, samples, acc.data_ptr(), aov.data_ptr(), rgb_ptr=rgb.data_ptr(), rgba_ptr=rgba.data_ptr(),
                var_ptr=var.data_ptr(), counts_ptr=None if cnt is None else cnt.data_ptr(),
                stream=None if stream is None else stream.cuda_stream, **params)
    hip.sync()
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), rgba.cpu().numpy(), var.cpu().numpy()


def check(hip, w, h, samples, acc, aov, counts=None, what="", **params):
    """The device's three outputs against the restatement, on the bits."""
    npy = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    rgb, rgba, var = run(hip, w, h, samples, acc, aov, counts, **params)
    want_rgb, want_var = SE.denoise(npy(acc), npy(aov), w, h, samples, None if counts is None else npy(counts), **params)
    assert same(rgb, want_rgb), f"{what}: rgb differs at {int((bits(rgb) != bits(want_rgb)).any(axis=1).sum())} pixels"
    assert same(var, want_var), f"{what}: variance differs at {int((bits(var) != bits(want_var)).sum())} pixels"
    ok = np.isfinite(rgb).all(axis=1)   # (the 8-bit value of a NaN is not defined)
    assert np.array_equal(rgba[ok], DE.film_rgba8(rgb)[ok]), f"{what}: rgba"
    return rgb, rgba, var


# ------------------------------------------------------------------ 1. small frames and count mixes
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
def test_small_frames_equal_the_restatement(hip, w, h, radius):
    """Levels 1 (the LDS level kernel follows the estimate) and 4 (the L2 one does too); per-pixel counts from
    {0, 1, 2, 3, 4, 9} with misses, a NaN and an infinity, and a whole frame of one sample without counts."""
    accum, aov, counts = mixed_frame(w, h)
    one = DE.synthetic_frame(w, h, 1, seed=5)
    for levels in (1, 4):
        for min_count in (2, 4):
            what = f"{w}x{h} r {radius} min_count {min_count} levels {levels}"
            check(hip, w, h, 0, accum, aov, counts, spatial=(min_count, radius), iterations=levels, what=what + " counts")
            check(hip, w, h, 1, one[0], one[1], spatial=(min_count, radius), iterations=levels, what=what + " one sample")
    check(hip, w, h, 0, accum, aov, counts, spatial=(4, radius), iterations=2, demodulate=False, what="not demodulated")


def test_the_estimate_changes_a_one_sample_frame_and_no_frame_of_many(hip):
    accum, aov, _ = DE.synthetic_frame(75, 41, 1, seed=3)
    ones = np.ones(75 * 41, np.int32)
    plain = run(hip, 75, 41, 0, accum, aov, ones, iterations=5)
    est = check(hip, 75, 41, 0, accum, aov, ones, spatial=(4, 1), iterations=5, what="one sample")
    assert not same(plain[0], est[0]) and not est[2].tolist() == plain[2].tolist()
    accum, aov, _ = DE.synthetic_frame(75, 41, 4, seed=3)
    plain = run(hip, 75, 41, 4, accum, aov, iterations=5)
    est = check(hip, 75, 41, 4, accum, aov, spatial=(4, 3), iterations=5, what="four samples")
    assert same(plain[0], est[0]) and same(plain[2], est[2]) and np.array_equal(plain[1], est[1])


# ------------------------------------------------------------------ 2. sv == NULL, the profile
def test_a_null_sv_is_the_plain_call_and_the_profiles(hip):
    accum, aov, _ = DE.synthetic_frame(40, 30, 8)
    n = 40 * 30
    acc = torch.from_numpy(accum).to(DEV)
    img = torch.from_numpy(aov).to(DEV)
    outs = [(torch.full((n, 3), NAN, dtype=torch.float32, device=DEV), torch.zeros((n, 4), dtype=torch.uint8, device=DEV),
             torch.full((n,), NAN, dtype=torch.float32, device=DEV)) for _ in range(3)]
    torch.cuda.synchronize()
    p = capi.Denoise(40, 30, 4, 1, 4.0, 0.4, 1.0)
    hip.set_profiling(2)   # (2: with the work counters, for the algorithmic bytes)
    rgb, rgba, var = outs[0]
    assert hip.lib.pbr_hip_denoise(hip.ctx, C.byref(p), 8, None, acc.data_ptr(), img.data_ptr(), rgb.data_ptr(), rgba.data_ptr(),
                                   var.data_ptr(), None) == capi.PBR_OK
    plain = hip.get_profile()
    rgb, rgba, var = outs[1]
    assert hip.lib.pbr_hip_denoise_sv(hip.ctx, C.byref(p), None, 8, None, acc.data_ptr(), img.data_ptr(), rgb.data_ptr(),
                                      rgba.data_ptr(), var.data_ptr(), None) == capi.PBR_OK
    null_sv = hip.get_profile()
    sv = capi.SpatialVariance(4, 2)
    rgb, rgba, var = outs[2]
    assert hip.lib.pbr_hip_denoise_sv(hip.ctx, C.byref(p), C.byref(sv), 8, None, acc.data_ptr(), img.data_ptr(), rgb.data_ptr(),
                                      rgba.data_ptr(), var.data_ptr(), None) == capi.PBR_OK
    with_sv = hip.get_profile()
    hip.set_profiling(False)
    torch.cuda.synchronize()
    names = ["k_dn_atrous_l0", "k_dn_atrous_l1", "k_dn_atrous_l2", "k_dn_atrous_l3", "k_dn_finish", "k_dn_prepare"]
    assert sorted(plain) == names and sorted(null_sv) == names
    assert sorted(with_sv) == sorted(names + ["k_dn_spatial"])
    assert all(v["launches"] == 1 for v in with_sv.values()) and all(v["launches"] == 1 for v in null_sv.values())
    assert with_sv["k_dn_spatial"]["units"] == n and with_sv["k_dn_spatial"]["bytes"] == 68 * n
    assert {k: (v["units"], v["bytes"]) for k, v in plain.items()} == {k: (v["units"], v["bytes"]) for k, v in null_sv.items()}
    # (the third call: 8 samples everywhere, so no pixel takes the estimate and the levels, started from the
    # other plane, give the plain call's bits)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a, b) if a.dtype == np.uint8 else same(a, b)
    want = DE.denoise(accum, aov, 40, 30, 8, iterations=4)
    assert same(outs[0][0].cpu().numpy(), want[0])


def test_the_library_refuses_what_the_wrapper_refuses(hip):
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    a = buf.data_ptr()
    good = dict(width=4, height=2, iterations=2, demodulate=1, sigma_l=4.0, sigma_n=0.4, sigma_z=1.0)

    def rc(samples=1, counts=None, sv=(4, 1), accum=a, aov=a, rgb=a, **change):
        p = capi.Denoise(**{**good, **change})
        s = None if sv is None else C.byref(capi.SpatialVariance(*sv))
        return hip.lib.pbr_hip_denoise_sv(hip.ctx, C.byref(p), s, samples, counts, accum, aov, rgb, None, None, None)

    assert rc() == capi.PBR_OK
    assert rc(sv=(2, 3)) == capi.PBR_OK and rc(sv=(64, 2)) == capi.PBR_OK and rc(samples=0, counts=a) == capi.PBR_OK
    hip.sync()
    for bad in (dict(sv=(1, 1)), dict(sv=(65, 1)), dict(sv=(4, 0)), dict(sv=(4, 4)), dict(sv=(-1, -1)), dict(samples=0),
                dict(samples=-3), dict(sv=None), dict(sv=None, samples=0), dict(accum=None), dict(aov=None), dict(rgb=None),
                dict(width=0), dict(iterations=9), dict(sigma_n=NAN)):
        assert rc(**bad) == capi.PBR_E_INVALID, bad
    assert rc(sv=None, samples=2) == capi.PBR_OK
    hip.sync()


# ------------------------------------------------------------------ 3. repeatability, streams, a growing frame
def test_two_calls_and_another_stream_give_the_same_bits(hip):
    accum, aov, counts = mixed_frame(70, 21)
    kw = dict(spatial=(4, 2), iterations=4)
    first = run(hip, 70, 21, 0, accum, aov, counts, **kw)
    again = run(hip, 70, 21, 0, accum, aov, counts, **kw)
    s2 = torch.cuda.Stream(DEV)
    other = run(hip, 70, 21, 0, accum, aov, counts, stream=s2, **kw)
    for a, b, c in zip(first, again, other):
        if a.dtype == np.uint8:
            ok = np.isfinite(first[0]).all(axis=1)
            assert np.array_equal(a[ok], b[ok]) and np.array_equal(a[ok], c[ok])
        else:
            assert same(a, b) and same(a, c)
    # a larger frame after a smaller one grows the fifth plane with the others
    big = DE.synthetic_frame(200, 130, 1)
    check(hip, 200, 130, 1, big[0], big[1], spatial=(4, 3), iterations=2, what="grown")
    assert same(run(hip, 70, 21, 0, accum, aov, counts, **kw)[0], first[0]), "the small frame in the larger planes"


# ------------------------------------------------------------------ 4. a rendered frame at one sample
def test_the_first_temporal_frame_at_one_sample(hip):
    """TemporalRender(samples_per_frame=1), first frame: every pixel has a count of 1.  denoise(spatial=...)
    equals the restatement on history()'s buffers and differs from denoise(), which can filter nothing.
    Statistical, not on the bits: against the same camera's 512 spp render its squared error (summed in float64)
    is below denoise()'s; the figures are printed."""
    s, rd = scene(hip)
    d = path_desc(rd, 64)
    t = TemporalRender(hip, d, 1)
    t.frame(d.camera)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in t.history().items()}
    assert (h["counts"] == 1).all()
    plain = t.denoise()[0].clone()
    est = t.denoise(spatial=(4, 1))[0].clone()
    torch.cuda.synchronize()
    plain, est = plain.cpu().numpy(), est.cpu().numpy()
    want, _ = SE.denoise(h["accum"], h["features"], W, H, 0, h["counts"], spatial=(4, 1))
    assert same(est, want)
    assert same(plain, DE.denoise(h["accum"], h["features"], W, H, 0, h["counts"])[0])
    assert not same(est, plain)
    ref, _, _ = hip.render(path_desc(rd, 512))
    err = lambda img: float(((img.astype(np.float64) - ref.astype(np.float64)) ** 2).sum())
    e_in, e_plain, e_est = err(h["accum"][:, :3]), err(plain), err(est)
    print(f"squared error against 512 spp: one sample {e_in:.6g}, denoise() {e_plain:.6g}, denoise(spatial=(4, 1)) "
          f"{e_est:.6g}, ratio {e_est / e_plain:.4f}")
    assert np.isfinite(est).all()
    assert e_est < e_plain


# ------------------------------------------------------------------ 5. the Python layer
def test_progressive_denoise_after_one_sample(hip):
    s, rd = scene(hip)
    p = ProgressiveRender(hip, path_desc(rd, 8), features=True)
    p.step(1)
    with pytest.raises(ValueError, match="at least 2 samples"):
        p.denoise()
    rgb, rgba = p.denoise(spatial=(4, 2), iterations=3)
    torch.cuda.synchronize()
    acc, img = p._accum.cpu().numpy(), p._aov_img.cpu().numpy()
    want, _ = SE.denoise(acc, img, W, H, 1, spatial=(4, 2), iterations=3)
    assert rgb.shape == (W * H, 3) and rgba.shape == (W * H, 4)
    assert same(rgb.cpu().numpy(), want)
    assert not same(want, acc[:, :3]), "the filter should have changed the image"
    ok = np.isfinite(want).all(axis=1)
    assert np.array_equal(rgba.cpu().numpy()[ok], DE.film_rgba8(want)[ok])
