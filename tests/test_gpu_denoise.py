"""pbr_hip_denoise on the device: the edge-avoiding à-trous filter over the pass sums and the feature image.

Every comparison is on the bits (uint32 views) against denoise_expected.py, the numpy restatement of the
rule, over inputs copied back from the device; rgba against the restated film transform of the device's
own rgb.  The one statistical test (quality on a render) says so."""
import numpy as np
import pytest
import torch

import denoise_expected as DE
from pysicalbasedraytracer_amd import HipRenderer, ProgressiveRender, capi, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
NAN, INF = float("nan"), float("inf")
W, H, SPP = 64, 36, 8


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


def path_desc(rd, spp):
    return scenes.render_desc(rd.camera, capi.INTEGRATOR_PATH, spp, rd.max_depth, rd.rr_threshold, rd.light_strategy,
                              capi.SAMPLER_HALTON)


_frame = {}


def rendered(hip):
    """The small C4-style Path scene (glass, metal, plastic, matte under an area light) at 64x36, 8 spp
    Halton: (scene, descriptor, pass sums, feature image) with the buffers as device tensors, rendered once
    and left unchanged."""
    if not _frame:
        s, rd = scenes.config_c4(W, H, SPP, mesh=small_dragon(40))
        rd = path_desc(rd, SPP)
        hip.upload(s)
        acc = torch.zeros((W * H, 6), dtype=torch.float32, device=DEV)
        facc = torch.zeros((W * H, 8), dtype=torch.float32, device=DEV)
        fimg = torch.zeros((W * H, 8), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        hip.render_passes(rd, 0, SPP, acc.data_ptr(), [None], [None])
        hip.render_aov(rd, 0, SPP, facc.data_ptr(), fimg.data_ptr())
        hip.sync()
        _frame.update(scene=s, rd=rd, acc=acc, fimg=fimg)
    return _frame["scene"], _frame["rd"], _frame["acc"], _frame["fimg"]


def run(hip, w, h, samples, acc, aov, counts=None, stream=None, outputs=("rgb", "rgba", "var"), **params):
    """One denoise call over device tensors (numpy inputs are uploaded); NaN / zero-filled outputs back as
    numpy: (rgb [n, 3], rgba [n, 4], var [n]), None for an output not asked for."""
    dev = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    acc, aov = dev(acc, np.float32), dev(aov, np.float32)
    cnt = None if counts is None else dev(counts, np.int32)
    n = w * h
    rgb = torch.full((n, 3), NAN, dtype=torch.float32, device=DEV) if "rgb" in outputs else None
    rgba = torch.zeros((n, 4), dtype=torch.uint8, device=DEV) if "rgba" in outputs else None
    var = torch.full((n,), NAN, dtype=torch.float32, device=DEV) if "var" in outputs else None
    torch.cuda.synchronize()   # (uploads and fills run on torch's stream, the call on its own)
    ptr = lambda t: None if t is None else t.data_ptr()
    hip.denoise(w, h, samples, acc.data_ptr(), aov.data_ptr(), rgb_ptr=ptr(rgb), rgba_ptr=ptr(rgba), var_ptr=ptr(var),
                counts_ptr=ptr(cnt), stream=None if stream is None else stream.cuda_stream, **params)
    hip.sync()
    torch.cuda.synchronize()
    back = lambda t: None if t is None else t.cpu().numpy()
    return back(rgb), back(rgba), back(var)


def check(hip, w, h, samples, acc, aov, counts=None, what="", **params):
    """The device's three outputs against the restatement, on the bits."""
    npy = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    rgb, rgba, var = run(hip, w, h, samples, acc, aov, counts, **params)
    want_rgb, want_var = DE.denoise(npy(acc), npy(aov), w, h, samples, None if counts is None else npy(counts), **params)
    assert same(rgb, want_rgb), f"{what}: rgb differs at {int((bits(rgb) != bits(want_rgb)).any(axis=1).sum())} pixels"
    assert same(var, want_var), f"{what}: variance differs at {int((bits(var) != bits(want_var)).sum())} pixels"
    ok = np.isfinite(rgb).all(axis=1)   # (the 8-bit value of a NaN is not defined)
    assert np.array_equal(rgba[ok], DE.film_rgba8(rgb)[ok]), f"{what}: rgba"
    return rgb, rgba, var


# ------------------------------------------------------------------ 1. a rendered frame
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_a_rendered_path_frame_equals_the_restatement(hip, levels, demodulate):
    s, rd, acc, fimg = rendered(hip)
    a = acc.cpu().numpy()
    assert np.isfinite(a).all() and (a[:, :3] > 0).any(), "the frame should hold light"
    cov = fimg.cpu().numpy()[:, 3]
    assert 0 < cov.sum() < cov.size, "the frame should hold hits and misses"
    rgb, _, var = check(hip, W, H, SPP, acc, fimg, iterations=levels, demodulate=demodulate, what=f"{levels} levels")
    assert np.isfinite(rgb).all() and np.isfinite(var).all()
    assert not same(rgb, a[:, :3] / f32(SPP)), "the filter should have changed the image"


# ------------------------------------------------------------------ 2. shapes where a tiled stencil goes wrong
@pytest.mark.parametrize("w,h,levels", [(37, 23, 3), (8, 5, 5), (1, 1, 2), (70, 3, 4), (3, 70, 4), (33, 9, 2)],
                         ids=lambda v: str(v))
def test_awkward_shapes(hip, w, h, levels):
    """A multiple of no tile size; steps beyond the frame; one pixel; strips one tile high or wide whose
    halo is mostly outside the frame; one pixel past a tile in both directions."""
    accum, aov, _ = DE.synthetic_frame(w, h, 8, seed=w * 100 + h)
    for demod in (False, True):
        check(hip, w, h, 8, accum, aov, iterations=levels, demodulate=demod, what=f"{w}x{h}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6])
def test_every_level_count_on_one_frame(hip, levels):
    """Levels 0 to 2 run the LDS variants (steps 1, 2, 4), the levels above the one that reads through L2,
    and the result lands in either plane of the ping-pong: every count up to 6 (step 32 on a 75-pixel-wide
    frame)."""
    accum, aov, _ = DE.synthetic_frame(75, 41, 8, seed=3)
    check(hip, 75, 41, 8, accum, aov, iterations=levels, what=f"{levels} levels")


# ------------------------------------------------------------------ 3. per-pixel counts
def test_counts_of_an_adaptive_render(hip):
    s, rd, _, fimg = rendered(hip)
    n = W * H
    acc = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    cnt = torch.zeros((n,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    res = hip.render_adaptive(path_desc(rd, 32), 4, 4, 0.05, 0.01, acc.data_ptr(), cnt.data_ptr())
    c = cnt.cpu().numpy()
    assert c.min() >= 4 and len(set(c.tolist())) > 1, "the adaptive render should leave differing counts"
    check(hip, W, H, 0, acc, fimg, counts=cnt, iterations=3, what="adaptive counts")
    # ... and counts of 0 and 1 on a few pixels (their sums: none, and one sample's)
    a = acc.cpu().numpy().copy()
    for p, k in ((0, 0), (W + 5, 1), (n // 2, 0), (n - 1, 1)):
        c[p] = k
        a[p] = 0 if k == 0 else np.concatenate([a[p, :3] / f32(8), (a[p, :3] / f32(8)) ** 2])
    rgb, _, var = check(hip, W, H, 0, a, fimg, counts=c, iterations=3, what="counts of 0 and 1")
    assert np.isfinite(rgb).all() and np.isfinite(var).all()


# ------------------------------------------------------------------ 4. NaN, infinite sigmas
def test_one_nan_colour_stays_on_its_pixel(hip):
    accum, aov, _ = DE.synthetic_frame(40, 30, 8)
    p = 13 * 40 + 17
    accum[p, 1] = NAN
    for levels in (1, 4):
        rgb, _, var = check(hip, 40, 30, 8, accum, aov, iterations=levels, what="NaN colour")
        bad = np.isnan(rgb).any(axis=1)
        assert bad.sum() == 1 and bad[p], f"{int(bad.sum())} NaN pixels"
        assert np.isfinite(var).all()


def test_infinite_sigmas_give_the_plain_wavelet(hip):
    """Every edge-stopping term switched off: e = 0 and w = 1 on every tap, the plain B3 à-trous wavelet
    renormalised at the frame's border; a constant image comes back as it is."""
    accum, aov, _ = DE.synthetic_frame(48, 20, 8)
    off = dict(sigma_l=INF, sigma_n=INF, sigma_z=INF)
    rgb, _, _ = check(hip, 48, 20, 8, accum, aov, iterations=3, demodulate=False, what="plain wavelet", **off)
    assert not same(rgb, check(hip, 48, 20, 8, accum, aov, iterations=3, demodulate=False)[0])
    flat = np.zeros_like(accum)
    flat[:, :3], flat[:, 3:] = 8 * 0.75, 8 * 0.75 * 0.75
    rgb, _, var = run(hip, 48, 20, 8, flat, aov, iterations=5, demodulate=False, **off)
    assert same(rgb, np.full_like(rgb, 0.75)) and not var.any()


# ------------------------------------------------------------------ 5. repeatability, streams, outputs
def test_two_calls_and_another_stream_give_the_same_bits(hip):
    s, rd, acc, fimg = rendered(hip)
    first = run(hip, W, H, SPP, acc, fimg, iterations=5)
    again = run(hip, W, H, SPP, acc, fimg, iterations=5)
    assert all(np.array_equal(bits(a) if a.dtype != np.uint8 else a, bits(b) if b.dtype != np.uint8 else b)
               for a, b in zip(first, again))
    # a call on one stream, a reader on another ordered behind it by wait_frame
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    rgb = torch.full((W * H, 3), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.denoise(W, H, SPP, acc.data_ptr(), fimg.data_ptr(), rgb_ptr=rgb.data_ptr(), iterations=5, stream=s1.cuda_stream)
    hip.wait_frame(s2.cuda_stream, 0)
    with torch.cuda.stream(s2):
        copy = rgb.clone()
    s2.synchronize()
    assert same(copy.cpu().numpy(), first[0])
    # ... and a second call on the other stream (the context's planes: drained first)
    rgb2 = torch.full((W * H, 3), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hip.denoise(W, H, SPP, acc.data_ptr(), fimg.data_ptr(), rgb_ptr=rgb2.data_ptr(), iterations=5, stream=s2.cuda_stream)
    hip.sync()
    torch.cuda.synchronize()
    assert same(rgb2.cpu().numpy(), first[0])


def test_each_output_alone_and_a_growing_frame(hip):
    """Any one output may be asked for alone; a larger frame after a smaller one grows the planes."""
    accum, aov, _ = DE.synthetic_frame(20, 10, 8)
    rgb, rgba, var = run(hip, 20, 10, 8, accum, aov, iterations=2)
    assert same(run(hip, 20, 10, 8, accum, aov, iterations=2, outputs=("rgb",))[0], rgb)
    assert np.array_equal(run(hip, 20, 10, 8, accum, aov, iterations=2, outputs=("rgba",))[1], rgba)
    assert same(run(hip, 20, 10, 8, accum, aov, iterations=2, outputs=("var",))[2], var)
    big = DE.synthetic_frame(200, 130, 8)
    check(hip, 200, 130, 8, big[0], big[1], iterations=2, what="grown")
    assert same(run(hip, 20, 10, 8, accum, aov, iterations=2)[0], rgb), "the small frame in the larger planes"


def test_the_library_refuses_what_the_wrapper_refuses(hip):
    import ctypes as C
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    a = buf.data_ptr()
    good = dict(width=4, height=2, iterations=2, demodulate=1, sigma_l=4.0, sigma_n=0.4, sigma_z=1.0)

    def rc(samples=8, counts=None, accum=a, aov=a, rgb=a, rgba=None, var=None, **change):
        p = capi.Denoise(**{**good, **change})
        return hip.lib.pbr_hip_denoise(hip.ctx, C.byref(p), samples, counts, accum, aov, rgb, rgba, var, None)

    assert rc() == capi.PBR_OK
    hip.sync()
    assert hip.lib.pbr_hip_denoise(hip.ctx, None, 8, None, a, a, a, None, None, None) == capi.PBR_E_INVALID
    for bad in (dict(accum=None), dict(aov=None), dict(rgb=None), dict(width=0), dict(height=-1),
                dict(width=1 << 16, height=1 << 15), dict(iterations=0), dict(iterations=9), dict(sigma_l=0.0),
                dict(sigma_n=NAN), dict(sigma_z=-1.0), dict(samples=1), dict(samples=0)):
        assert rc(**bad) == capi.PBR_E_INVALID, bad
    assert rc(samples=1, counts=a) == capi.PBR_OK   # (per-pixel counts: `samples` is not read)
    hip.sync()


# ------------------------------------------------------------------ 6. the Python layer
def test_progressive_denoise_equals_the_call_on_its_buffers(hip):
    s, rd, acc, fimg = rendered(hip)
    p = ProgressiveRender(hip, rd, features=True)
    p.step(4)
    p.step(4)
    rgb, rgba = p.denoise(iterations=3, sigma_l=2.0)
    torch.cuda.synchronize()
    assert same(p._accum.cpu().numpy(), acc.cpu().numpy()) and same(p._aov_img.cpu().numpy(), fimg.cpu().numpy())
    want = run(hip, W, H, SPP, acc, fimg, iterations=3, sigma_l=2.0)
    assert rgb.shape == (W * H, 3) and rgba.shape == (W * H, 4)
    assert same(rgb.cpu().numpy(), want[0]) and np.array_equal(rgba.cpu().numpy(), want[1])
    assert not same(p._rgb.cpu().numpy(), want[0]), "the step's own image is left as it was"


def test_the_profile_names_each_level(hip):
    accum, aov, _ = DE.synthetic_frame(40, 30, 8)
    hip.set_profiling(True)
    run(hip, 40, 30, 8, accum, aov, iterations=4)
    prof = hip.get_profile()
    hip.set_profiling(False)
    assert sorted(prof) == ["k_dn_atrous_l0", "k_dn_atrous_l1", "k_dn_atrous_l2", "k_dn_atrous_l3", "k_dn_finish", "k_dn_prepare"]
    assert all(v["launches"] == 1 for v in prof.values())


# ------------------------------------------------------------------ 7. quality on a render
def test_the_denoised_frame_is_closer_to_the_converged_render(hip):
    """Statistical, not on the bits: the 8 spp frame denoised at 5 levels against the same scene's 512 spp
    render, both squared errors summed in float64.  The denoised error must be strictly below the noisy
    one; the ratio is printed."""
    s, rd, acc, fimg = rendered(hip)
    ref, _, _ = hip.render(path_desc(rd, 512))
    noisy = acc.cpu().numpy()[:, :3] / f32(SPP)
    rgb, _, _ = run(hip, W, H, SPP, acc, fimg, iterations=5)
    e_noisy = float(((noisy.astype(np.float64) - ref.astype(np.float64)) ** 2).sum())
    e_dn = float(((rgb.astype(np.float64) - ref.astype(np.float64)) ** 2).sum())
    print(f"squared error against 512 spp: noisy {e_noisy:.6g}, denoised {e_dn:.6g}, ratio {e_dn / e_noisy:.4f}")
    assert e_dn < e_noisy
