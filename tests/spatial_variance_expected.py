"""The denoiser's spatial variance estimate restated in numpy: the rule of DESIGN §4.9 on top of
denoise_expected.py (prepare, level), float32 throughout and in the stated order, one whole-image array
operation per tap, so that it produces the bits pbr_hip_denoise_sv and pbr_hip_spatial_variance_host
produce.  Inputs as denoise_expected takes them.  No GPU, no library."""
import numpy as np

import denoise_expected as DE

f32 = np.float32
FMAX = np.finfo(np.float32).max


def _counts(width, height, samples, counts):
    W, H = int(width), int(height)
    return np.full((H, W), int(samples), np.int64) if counts is None else np.asarray(counts, np.int64).reshape(H, W)


@DE._quiet
def moments(accum, width, height, samples, counts, b):
    """(u [H, W, 3], n [H, W]): the per-sample second moment in the filter's domain, (Q / n) / (b b), and the
    count as float32; both 0 where the count is below 1."""
    W, H = int(width), int(height)
    k = _counts(W, H, samples, counts)
    Q = np.ascontiguousarray(accum, dtype=f32).reshape(H, W, 6)[..., 3:6]
    n = k.astype(f32)
    u = (Q / n[..., None]) / (b * b)
    has = k >= 1
    return np.where(has[..., None], u, f32(0)).astype(f32), np.where(has, n, f32(0)).astype(f32)


@DE._quiet
def estimate(x, V, N, z, g, u, n, min_count, radius, in_, iz):
    """The variance plane after the estimate: V where a pixel keeps prepare's value, the pooled estimate where
    1 <= count < min_count and the kept taps hold at least two samples."""
    H, W = V.shape
    r = int(radius)
    zc = f32(1e-3) * z + f32(1e-6)
    fin = (np.abs(x) <= FMAX).all(-1) & (np.abs(u) <= FMAX).all(-1)   # (a NaN fails the comparison)
    usable = (n >= f32(1)) & fin
    sa = np.zeros((H, W), f32)
    s1 = np.zeros((H, W, 3), f32)
    s2 = np.zeros((H, W, 3), f32)
    kt = np.zeros((H, W), np.int64)
    kq = n.astype(np.int64)
    for j in range(-r, r + 1):
        py = slice(max(0, -j), min(H, H - j))   # the pixels p whose tap q = p + (i, j) lies in the frame
        if py.start >= py.stop:
            continue
        qy = slice(py.start + j, py.stop + j)
        for i in range(-r, r + 1):
            px = slice(max(0, -i), min(W, W - i))
            if px.start >= px.stop:
                continue
            qx = slice(px.start + i, px.stop + i)
            P, Qq = (py, px), (qy, qx)
            keep = usable[Qq]
            if i == 0 and j == 0:
                w = np.ones(V[P].shape, f32)
            else:
                dN = N[P] - N[Qq]
                en = ((dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]) * in_
                dz = z[P] - z[Qq]
                den = g[P] * f32(max(abs(i), abs(j))) + zc[P]
                ez = ((dz * dz) / (den * den)) * iz
                e = en + ez
                keep = keep & (e < f32(16))
                t = f32(1) - e * f32(0.0625)
                t = t * t
                t = t * t
                t = t * t
                t = t * t
                w = t
            a = w * n[Qq]
            sa[P] = np.where(keep, sa[P] + a, sa[P])
            s1[P] = np.where(keep[..., None], s1[P] + a[..., None] * x[Qq], s1[P])
            s2[P] = np.where(keep[..., None], s2[P] + a[..., None] * u[Qq], s2[P])
            kt[P] = np.where(keep, kt[P] + kq[Qq], kt[P])
    M = s1 / sa[..., None]
    U = s2 / sa[..., None]
    d = U - M * M
    sig = np.where(d > 0, d, f32(0)).astype(f32)
    est = ((sig[..., 0] + sig[..., 1]) + sig[..., 2]) / n
    takes = (n >= f32(1)) & (n < f32(min_count)) & (kt >= 2)
    return np.where(takes, est, V).astype(f32)


def _sigmas(sigma_l, sigma_n, sigma_z):
    return (f32(1) / (f32(sigma_l) * f32(sigma_l)), f32(1) / (f32(sigma_n) * f32(sigma_n)),
            f32(1) / (f32(sigma_z) * f32(sigma_z)))


@DE._quiet
def variance(accum, aov, width, height, samples, counts=None, spatial=(4, 1), demodulate=True, sigma_n=0.4, sigma_z=1.0):
    """[n] float32 of pbr_hip_spatial_variance_host: V after prepare and the estimate (spatial=None: after prepare)."""
    _, in_, iz = _sigmas(1.0, sigma_n, sigma_z)
    x, V, N, z, g, b = DE.prepare(accum, aov, width, height, samples, counts, demodulate)
    if spatial is not None:
        u, n = moments(accum, width, height, samples, counts, b)
        V = estimate(x, V, N, z, g, u, n, spatial[0], spatial[1], in_, iz)
    return V.reshape(-1)


@DE._quiet
def denoise(accum, aov, width, height, samples, counts=None, spatial=(4, 1), iterations=5, demodulate=True, sigma_l=4.0,
            sigma_n=0.4, sigma_z=1.0):
    """(rgb [n, 3] float32, var [n] float32) of pbr_hip_denoise_sv; spatial=None: of pbr_hip_denoise."""
    il, in_, iz = _sigmas(sigma_l, sigma_n, sigma_z)
    x, V, N, z, g, b = DE.prepare(accum, aov, width, height, samples, counts, demodulate)
    if spatial is not None:
        u, n = moments(accum, width, height, samples, counts, b)
        V = estimate(x, V, N, z, g, u, n, spatial[0], spatial[1], in_, iz)
    for i in range(int(iterations)):
        x, V = DE.level(x, V, N, z, g, 1 << i, il, in_, iz)
    return (x * b).astype(f32).reshape(-1, 3), V.reshape(-1)
