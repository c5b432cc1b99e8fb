"""pbr_hip_denoise restated in numpy: the rule of DESIGN §4.5, float32 throughout and in the stated
order, one whole-image array operation per tap, so that it produces the bits the device produces.

Inputs as the C-ABI takes them, over a width x height frame in raster order: accum [n, 6] (the sums of
render_passes), aov [n, 8] (the image of render_aov), counts [n] int32 or None.  No GPU, no library."""
import numpy as np

f32 = np.float32
K3 = (f32(0.25), f32(0.5), f32(0.25))
H5 = (f32(0.375), f32(0.25), f32(0.0625))


def _quiet(fn):
    def run(*a, **k):
        with np.errstate(all="ignore"):   # (0/0, inf - inf and overflow are part of the rule: NaN drops a tap)
            return fn(*a, **k)
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


@_quiet
def prepare(accum, aov, width, height, samples, counts=None, demodulate=True):
    """(x [H, W, 3], V [H, W], N [H, W, 3], z [H, W], g [H, W], b [H, W, 3]) of the prepare step."""
    W, H = int(width), int(height)
    a = np.ascontiguousarray(accum, dtype=f32).reshape(H, W, 6)
    f = np.ascontiguousarray(aov, dtype=f32).reshape(H, W, 8)
    k = np.full((H, W), int(samples), np.int64) if counts is None else np.asarray(counts, np.int64).reshape(H, W)
    n = k.astype(f32)[..., None]
    S, Q = a[..., 0:3], a[..., 3:6]
    m2 = S / n
    d = Q - S * m2
    v2 = np.where(d > 0, d, f32(0)) / (n * (n - f32(1)))
    two = (k >= 2)[..., None]
    one = (k == 1)[..., None]
    m = np.where(two, m2, np.where(one, S, f32(0))).astype(f32)
    v = np.where(two, v2, f32(0)).astype(f32)
    if demodulate:
        al = f[..., 0:3] + (f32(1) - f[..., 3:4])
        b = np.where(al > f32(0.01), al, f32(0.01)).astype(f32)
    else:
        b = np.ones((H, W, 3), f32)
    x = (m / b).astype(f32)
    t = v / (b * b)
    V = ((t[..., 0] + t[..., 1]) + t[..., 2]).astype(f32)
    N, z = f[..., 4:7].copy(), f[..., 7].copy()
    xs, ys = np.arange(W), np.arange(H)
    xl, xr = np.clip(xs - 1, 0, W - 1), np.clip(xs + 1, 0, W - 1)
    yu, yd = np.clip(ys - 1, 0, H - 1), np.clip(ys + 1, 0, H - 1)
    gx = np.abs(z[:, xr] - z[:, xl])
    gy = np.abs(z[yd, :] - z[yu, :])
    g = (np.where(gx > gy, gx, gy) * f32(0.5)).astype(f32)
    return x, V, N, z, g, b


@_quiet
def level(x, V, N, z, g, s, il, in_, iz):
    """One wavelet level of step s over the previous level's x and V: the new (x, V)."""
    H, W = V.shape
    xs, ys = np.arange(W), np.arange(H)
    l = (x[..., 0] + x[..., 1]) + x[..., 2]
    vb = np.zeros((H, W), f32)
    for j in (-1, 0, 1):
        qy = np.clip(ys + j, 0, H - 1)
        for i in (-1, 0, 1):
            qx = np.clip(xs + i, 0, W - 1)
            vb = vb + (K3[j + 1] * K3[i + 1]) * V[qy[:, None], qx[None, :]]
    D = vb + f32(1e-8)
    zc = f32(1e-3) * z + f32(1e-6)
    sw = np.zeros((H, W), f32)
    sx = np.zeros((H, W, 3), f32)
    sv = np.zeros((H, W), f32)
    for j in range(-2, 3):
        dy = s * j
        py = slice(max(0, -dy), min(H, H - dy))   # the pixels p whose tap q = p + (dx, dy) lies in the frame
        if py.start >= py.stop:
            continue
        qy = slice(py.start + dy, py.stop + dy)
        for i in range(-2, 3):
            dx = s * i
            px = slice(max(0, -dx), min(W, W - dx))
            if px.start >= px.stop:
                continue
            qx = slice(px.start + dx, px.stop + dx)
            P, Qq = (py, px), (qy, qx)
            hh = H5[abs(i)] * H5[abs(j)]
            if i == 0 and j == 0:
                keep = np.ones(V[P].shape, bool)
                hw = np.full(V[P].shape, hh * f32(1), f32)
            else:
                dl = l[P] - l[Qq]
                el = ((dl * dl) / D[P]) * il
                dN = N[P] - N[Qq]
                en = ((dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]) * in_
                dz = z[P] - z[Qq]
                den = g[P] * f32(s * max(abs(i), abs(j))) + zc[P]
                ez = ((dz * dz) / (den * den)) * iz
                e = (el + en) + ez
                keep = e < f32(16)
                t = f32(1) - e * f32(0.0625)
                t = t * t
                t = t * t
                t = t * t
                t = t * t
                hw = hh * t
            sw[P] = np.where(keep, sw[P] + hw, sw[P])
            sx[P] = np.where(keep[..., None], sx[P] + hw[..., None] * x[Qq], sx[P])
            sv[P] = np.where(keep, sv[P] + (hw * hw) * V[Qq], sv[P])
    return (sx / sw[..., None]).astype(f32), (sv / (sw * sw)).astype(f32)


def film_rgba8(rgb):
    """The film transform of a render (XYZ round trip, sRGB curve, 8 bits) on float32 colours [n, 3]."""
    c = np.ascontiguousarray(rgb, dtype=f32).reshape(-1, 3)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(all="ignore"):
        X = f32(0.412453) * r + f32(0.357580) * g + f32(0.180423) * b
        Y = f32(0.212671) * r + f32(0.715160) * g + f32(0.072169) * b
        Z = f32(0.019334) * r + f32(0.119193) * g + f32(0.950227) * b
        o = (f32(3.240479) * X - f32(1.537150) * Y - f32(0.498535) * Z,
             f32(-0.969256) * X + f32(1.875991) * Y + f32(0.041556) * Z,
             f32(0.055648) * X - f32(0.204043) * Y + f32(1.057311) * Z)
        out = np.full((c.shape[0], 4), 255, np.uint8)
        for k, v in enumerate(o):
            p = np.power(v.astype(np.float64), np.float64(f32(1) / f32(2.4))).astype(f32)
            gc = np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * p - f32(0.055))
            q = f32(255) * gc + f32(0.5)
            q = np.where(q < 0, f32(0), np.where(q > f32(255), f32(255), q))
            out[:, k] = np.nan_to_num(q, nan=0.0).astype(np.int32).astype(np.uint8)
    return out


def synthetic_frame(width=64, height=48, samples=8, seed=7):
    """A noisy test frame with a known truth: sky above (misses), a textured floor whose distance ramps
    below, a disc with curved normals in front; every sample is the truth times a gamma variate of mean 1.
    Returns (accum [n, 6], aov [n, 8], truth [n, 3]) as float32."""
    W, H = int(width), int(height)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    albedo = np.zeros((H, W, 3))
    hit = np.zeros((H, W))
    nrm = np.zeros((H, W, 3))
    dist = np.zeros((H, W))
    shade = np.ones((H, W))
    floor = yy >= H // 2
    check = ((xx // 4 + yy // 3) % 2).astype(bool)
    albedo[floor] = np.where(check[floor][:, None], (0.8, 0.7, 0.2), (0.2, 0.3, 0.7))
    hit[floor] = 1
    nrm[floor] = (0, 1, 0)
    dist[floor] = 2.0 + 10.0 * (H - yy[floor]) / H
    shade[floor] = 0.5 + 0.5 * (yy[floor] - H // 2) / (H - H // 2)
    cx, cy, rad = W * 0.55, H * 0.45, min(W, H) * 0.28
    u, v = (xx - cx) / rad, (yy - cy) / rad
    disc = u * u + v * v < 1
    w = np.sqrt(np.clip(1 - u * u - v * v, 0, 1))
    albedo[disc] = (0.9, 0.4, 0.3)
    hit[disc] = 1
    nrm[disc] = np.stack([u, -v, w], -1)[disc]
    dist[disc] = 3.0 - w[disc]
    shade[disc] = 0.2 + 0.8 * w[disc]
    truth = np.where(hit[..., None] > 0, albedo * shade[..., None], (0.3, 0.5, 0.9))
    L = truth[None] * rng.gamma(2.0, 0.5, size=(int(samples), H, W, 1))
    accum = np.concatenate([L.sum(0), (L * L).sum(0)], -1).reshape(-1, 6).astype(f32)
    aov = np.concatenate([albedo, hit[..., None], nrm, dist[..., None]], -1).reshape(-1, 8).astype(f32)
    return accum, aov, truth.reshape(-1, 3).astype(f32)


@_quiet
def denoise(accum, aov, width, height, samples, counts=None, iterations=5, demodulate=True, sigma_l=4.0, sigma_n=0.4,
            sigma_z=1.0):
    """(rgb [n, 3] float32, var [n] float32) of pbr_hip_denoise."""
    il = f32(1) / (f32(sigma_l) * f32(sigma_l))
    in_ = f32(1) / (f32(sigma_n) * f32(sigma_n))
    iz = f32(1) / (f32(sigma_z) * f32(sigma_z))
    x, V, N, z, g, b = prepare(accum, aov, width, height, samples, counts, demodulate)
    for i in range(int(iterations)):
        x, V = level(x, V, N, z, g, 1 << i, il, in_, iz)
    return (x * b).astype(f32).reshape(-1, 3), V.reshape(-1)
