"""pbr_hip_temporal restated in numpy: the rule of DESIGN §4.8, float32 throughout and in the stated order,
one whole-image array operation per step and tap, so that it produces the bits the device and the host
twin produce.

Inputs as the C-ABI takes them, over a width x height frame in raster order: accum [n, 6] (the sums of
render_passes), aov [n, 8] (the image of render_aov), counts [n] int32; cur and prev are the
(raster_to_world, world_to_raster, eye) triples of capi.camera_matrices for this frame's and the previous
frame's camera.  temporal() itself touches no GPU and no library; synthetic_frame() asks the library for a
camera's matrices (a host-only call)."""
import numpy as np

f32 = np.float32
MOTIONS = ("identity", "subpixel_pan", "pan_out", "dolly_in", "dolly_out", "roll90", "turned_round")


def _divisor(f, demodulate):
    if not demodulate:
        return np.ones(f.shape[:-1] + (3,), f32)
    al = f[..., 0:3] + (f32(1) - f[..., 3:4])
    return np.where(al > f32(0.01), al, f32(0.01)).astype(f32)


def temporal(width, height, samples, accum_cur, aov_cur, counts_prev, accum_prev, aov_prev, cur, prev, counts_cur=None,
             max_history=32, demodulate=True, tol_z=0.05, tol_n=0.1):
    """(accum_out [n, 6] float32, counts_out [n] int32, motion [n, 2] float32, took [n] bool) of pbr_hip_temporal;
    took marks the pixels that took history."""
    with np.errstate(all="ignore"):   # (0/0, inf - inf and overflow are part of the rule: they drop a tap or a pixel)
        return _temporal(width, height, samples, accum_cur, aov_cur, counts_prev, accum_prev, aov_prev, cur, prev, counts_cur,
                         max_history, demodulate, tol_z, tol_n)


def _temporal(width, height, samples, accum_cur, aov_cur, counts_prev, accum_prev, aov_prev, cur, prev, counts_cur, max_history,
              demodulate, tol_z, tol_n):
    W, H = int(width), int(height)
    a = np.ascontiguousarray(accum_cur, dtype=f32).reshape(H, W, 6)
    f = np.ascontiguousarray(aov_cur, dtype=f32).reshape(H, W, 8)
    ap = np.ascontiguousarray(accum_prev, dtype=f32).reshape(H, W, 6)
    fp = np.ascontiguousarray(aov_prev, dtype=f32).reshape(H, W, 8)
    cp = np.asarray(counts_prev, dtype=np.int64).reshape(H, W)
    k = np.full((H, W), int(samples), np.int64) if counts_cur is None else np.asarray(counts_cur, np.int64).reshape(H, W)
    R = np.asarray(cur[0], dtype=f32).reshape(16)
    E = np.asarray(cur[2], dtype=f32).reshape(3)
    M = np.asarray(prev[1], dtype=f32).reshape(16)
    EP = np.asarray(prev[2], dtype=f32).reshape(3)
    tol_z, tol_n = f32(tol_z), f32(tol_n)
    # A. position
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)
    cov, z = f[..., 3], f[..., 7]
    X = (R[0] * fx + R[1] * fy) + R[3]
    Y = (R[4] * fx + R[5] * fy) + R[7]
    Zc = (R[8] * fx + R[9] * fy) + R[11]
    Wc = (R[12] * fx + R[13] * fy) + R[15]
    gx, gy, gz = X / Wc - E[0], Y / Wc - E[1], Zc / Wc - E[2]
    ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
    Px, Py, Pz = E[0] + (gx / ln) * z, E[1] + (gy / ln) * z, E[2] + (gz / ln) * z
    # B. projection
    xp = ((M[0] * Px + M[1] * Py) + M[2] * Pz) + M[3]
    yp = ((M[4] * Px + M[5] * Py) + M[6] * Pz) + M[7]
    wp = ((M[12] * Px + M[13] * Py) + M[14] * Pz) + M[15]
    rx, ry = xp / wp, yp / wp
    proj = (cov > 0) & (wp > 0) & (rx >= 0) & (rx < f32(W)) & (ry >= 0) & (ry < f32(H))
    motion = np.zeros((H, W, 2), f32)
    motion[..., 0] = np.where(proj, rx - fx, f32(0))
    motion[..., 1] = np.where(proj, ry - fy, f32(0))
    ex, ey, ez = Px - EP[0], Py - EP[1], Pz - EP[2]
    zexp = np.sqrt((ex * ex + ey * ey) + ez * ez)
    tz = tol_z * zexp
    # C. taps
    u, v = rx - f32(0.5), ry - f32(0.5)
    x0f, y0f = np.floor(u), np.floor(v)
    tx, ty = u - x0f, v - y0f
    x0 = np.where(proj, x0f, f32(0)).astype(np.int64)
    y0 = np.where(proj, y0f, f32(0)).astype(np.int64)
    sw = np.zeros((H, W), f32)
    sm = np.zeros((H, W, 3), f32)
    sq = np.zeros((H, W, 3), f32)
    kmin = np.full((H, W), np.iinfo(np.int32).max, np.int64)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            ok = proj & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)   # (a gather that stays in the frame; masked by ok)
            b = (tx if i else f32(1) - tx) * (ty if j else f32(1) - ty)
            ok &= b > 0
            kq = cp[qy, qx]
            ok &= kq >= 1
            fq = fp[qy, qx]
            ok &= fq[..., 3] > 0
            ok &= np.abs(fq[..., 7] - zexp) <= tz
            dN = f[..., 4:7] - fq[..., 4:7]
            en = (dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]
            ok &= en <= tol_n
            nq = kq.astype(f32)[..., None]
            bq = _divisor(fq, demodulate)
            aq = ap[qy, qx]
            mu = (aq[..., 0:3] / nq) / bq
            nu = (aq[..., 3:6] / nq) / (bq * bq)
            ok &= np.isfinite(mu).all(axis=-1) & np.isfinite(nu).all(axis=-1)
            sw = np.where(ok, sw + b, sw)
            sm = np.where(ok[..., None], sm + b[..., None] * mu, sm)
            sq = np.where(ok[..., None], sq + b[..., None] * nu, sq)
            kmin = np.where(ok, np.minimum(kmin, kq), kmin)
    # D. merge
    took = proj & (sw > 0)
    kh = np.minimum(kmin, int(max_history))
    nh = kh.astype(f32)[..., None]
    bp = _divisor(f, demodulate)
    mh = (sm / sw[..., None]) * bp
    qh = (sq / sw[..., None]) * (bp * bp)
    out = a.copy()
    out[..., 0:3] = np.where(took[..., None], a[..., 0:3] + mh * nh, a[..., 0:3])
    out[..., 3:6] = np.where(took[..., None], a[..., 3:6] + qh * nh, a[..., 3:6])
    counts = np.where(took, k + kh, k).astype(np.int32)
    return out.reshape(-1, 6), counts.reshape(-1), motion.reshape(-1, 2), took.reshape(-1)


def image(accum_out, counts_out):
    """rgb_out of the call: the colour sums over the count, 0 where the count is 0."""
    s = np.ascontiguousarray(accum_out, dtype=f32).reshape(-1, 6)[:, 0:3]
    n = np.asarray(counts_out).reshape(-1)
    with np.errstate(all="ignore"):
        return np.where((n == 0)[:, None], f32(0), s / n.astype(f32)[:, None]).astype(f32)


# ------------------------------------------------------------------ synthetic frames with a known truth
def camera(width, height, eye=(0.0, 0.5, 2.0), look=(0.0, 0.0, -4.0), up=(0.0, 1.0, 0.0)):
    from pysicalbasedraytracer_amd import scenes
    return scenes.camera(int(width), int(height), eye, look, up)


def previous_camera(width, height, motion):
    """The previous frame's camera for one of MOTIONS; this frame's is camera(width, height)."""
    eye, look, up = np.array((0.0, 0.5, 2.0)), np.array((0.0, 0.0, -4.0)), (0.0, 1.0, 0.0)
    fwd = (look - eye) / np.linalg.norm(look - eye)
    if motion == "identity":
        pass
    elif motion == "subpixel_pan":     # 0.05 units sideways: a third of a pixel at 64 pixels across, 5 units away
        eye, look = eye + (0.05, 0, 0), look + (0.05, 0, 0)
    elif motion == "pan_out":          # sideways by far more than the frame shows at any distance in the scene
        eye, look = eye + (1000.0, 0, 0), look + (1000.0, 0, 0)
    elif motion == "dolly_in":         # the camera moved forward: the previous one stood further back
        eye = eye - 0.3 * fwd
    elif motion == "dolly_out":
        eye = eye + 0.3 * fwd
    elif motion == "roll90":
        up = (1.0, 0.0, 0.0)
    elif motion == "turned_round":     # the previous camera looked the other way
        look = eye - (look - eye)
    else:
        raise ValueError(motion)
    return camera(width, height, tuple(eye), tuple(look), up)


def synthetic_frame(cam, samples, seed):
    """A noisy frame of a fixed world under the pinhole camera `cam` (a capi.CameraDesc), ray cast in float64
    through the pixel centres: a checkered floor (y = -1), a wall (z = -8, |x| < 6, y < 3), a sphere (centre
    (0, 0, -4), radius 1), sky elsewhere.  Every sample is the truth times a gamma variate of mean 1.  Returns
    (accum [n, 6], aov [n, 8], truth [n, 3], matrices) with matrices = capi.camera_matrices(cam)."""
    from pysicalbasedraytracer_amd import capi
    mats = capi.camera_matrices(cam)
    W, H = cam.width, cam.height
    r2w, eye = mats[0].astype(np.float64), mats[2].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    pr = np.stack([xs + 0.5, ys + 0.5, np.zeros((H, W)), np.ones((H, W))], -1) @ r2w.T
    d = pr[..., :3] / pr[..., 3:4] - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.full((H, W), np.inf)
    albedo = np.zeros((H, W, 3))
    nrm = np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        # floor
        tf = (-1.0 - eye[1]) / d[..., 1]
        hit = (tf > 0) & np.isfinite(tf)
        pf = eye + d * np.where(hit, tf, 0)[..., None]
        chk = ((np.floor(pf[..., 0] / 0.75) + np.floor(pf[..., 2] / 0.75)) % 2).astype(bool)
        t = np.where(hit, tf, t)
        albedo[hit] = np.where(chk[hit][:, None], (0.8, 0.7, 0.2), (0.2, 0.3, 0.7))
        nrm[hit] = (0, 1, 0)
        # wall
        tw = (-8.0 - eye[2]) / d[..., 2]
        pw = eye + d * np.where(np.isfinite(tw), tw, 0)[..., None]
        hit = (tw > 0) & np.isfinite(tw) & (tw < t) & (np.abs(pw[..., 0]) < 6) & (pw[..., 1] < 3)
        t = np.where(hit, tw, t)
        albedo[hit] = (0.6, 0.6, 0.55)
        nrm[hit] = (0, 0, 1)
        # sphere
        c = np.array((0.0, 0.0, -4.0))
        oc = eye - c
        bq = (d * oc).sum(-1)
        disc = bq * bq - (oc @ oc - 1.0)
        ts = -bq - np.sqrt(np.where(disc > 0, disc, 0))
        hit = (disc > 0) & (ts > 0) & (ts < t)
        t = np.where(hit, ts, t)
        albedo[hit] = (0.9, 0.4, 0.3)
        nrm[hit] = ((eye + d * np.where(hit, ts, 0)[..., None] - c))[hit]
    hit = np.isfinite(t)
    light = np.array((0.4, 0.8, 0.45))
    light /= np.linalg.norm(light)
    shade = 0.25 + 0.75 * np.clip(nrm @ light, 0, 1)
    truth = np.where(hit[..., None], albedo * shade[..., None], (0.3, 0.5, 0.9))
    rng = np.random.default_rng(seed)
    L = truth[None] * rng.gamma(2.0, 0.5, size=(int(samples), H, W, 1))
    accum = np.concatenate([L.sum(0), (L * L).sum(0)], -1).reshape(-1, 6).astype(f32)
    aov = np.concatenate([albedo, hit[..., None].astype(np.float64), nrm, np.where(hit, t, 0)[..., None]], -1)
    return accum, aov.reshape(-1, 8).astype(f32), truth.reshape(-1, 3).astype(f32), mats


_pairs = {}


def synthetic_pair(w, h, k, motion, seed=1):
    """Consistent current and previous frames of the fixed world, the previous camera `motion` away from the
    current one: a dict with width, height, samples, accum_cur, aov_cur, truth, cur (matrices), accum_prev,
    aov_prev, counts_prev (k everywhere), prev (matrices).  Computed once per argument set; the arrays are
    shared and must be left unchanged (copy before planting anything)."""
    key = (int(w), int(h), int(k), motion, int(seed))
    if key not in _pairs:
        ac, fc, truth, cur = synthetic_frame(camera(w, h), k, seed)
        ap, fpv, _, prev = synthetic_frame(previous_camera(w, h, motion), k, seed + 1000)
        pair = dict(width=int(w), height=int(h), samples=int(k), accum_cur=ac, aov_cur=fc, truth=truth, cur=cur, accum_prev=ap,
                    aov_prev=fpv, counts_prev=np.full(int(w) * int(h), int(k), np.int32), prev=prev)
        for v in pair.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _pairs[key] = pair
    return _pairs[key]


def call_args(pair, **change):
    """The keyword arguments of temporal() (and of HipRenderer.temporal_host) for a pair."""
    kw = {n: pair[n] for n in ("width", "height", "samples", "accum_cur", "aov_cur", "counts_prev", "accum_prev", "aov_prev",
                               "cur", "prev")}
    kw.update(change)
    return kw
