"""Expected feature buffers with mirror bounces followed (pbr_hip_render_aov_mirrors).

Two parts, both float32 numpy with every operation in the order of the C++ source:

  mirror_step      the step itself: make_bsdf's frame (ss = normalize(dpdu), ts = cross(ns, ss) with the
                   cross in float64 and one narrowing per component, as pbr_math.h has it), to_local, the
                   mirror direction, to_world, the three refusals, offset_ray_origin with nextafter.
  sample_values    the chain, built from entry points that are pinned elsewhere, as aov_expected builds the
                   plain pass: aov_expected.camera_rays, each segment's hit record from pbr_hip_query
                   (p, p_error, n, ns, dpdu, wo, uv, prim), the step from mirror_step, the albedo from
                   aov_expected.material_albedo (or a caller's function of the hit records: textures).

Scenes without material-less primitives only (those are tested by properties).  Test infrastructure only."""
import numpy as np

import aov_expected as E
from pysicalbasedraytracer_amd import capi

f32 = np.float32
CH = 8
# pbr_surface_hit as 28 float32 words
W_HIT, W_PRIM, W_T = 0, 1, 2
W_P, W_PERR, W_N, W_NS, W_DPDU, W_WO, W_UV = slice(6, 9), slice(9, 12), slice(12, 15), slice(15, 18), slice(18, 21), slice(21, 24), slice(24, 26)


def _dot(a, b):
    """dot(f3, f3): a.x * b.x + a.y * b.y + a.z * b.z, left to right, each operation rounded to float32."""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


def _cross(a, b):
    """cross(f3, f3): products and difference in float64, one narrowing per component."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def _normalize(a):
    """normalize(f3): a / len(a), the division being a multiplication by 1 / len."""
    l2 = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(f32) + a[:, 2] * a[:, 2]).astype(f32)
    inv = (f32(1) / np.sqrt(l2).astype(f32)).astype(f32)
    return (a * inv[:, None]).astype(f32)


def offset_ray_origin(p, perr, n, w):
    """offset_ray_origin (Geometry.h:1470-1484): p moved along n by dot(|n|, pError), to w's side, then one
    float further from the surface in every coordinate that moved."""
    d = _dot(np.abs(n), perr)
    off = (d[:, None] * n).astype(f32)
    off = np.where((_dot(w, n) < 0)[:, None], -off, off)
    po = (p + off).astype(f32)
    up, down = np.nextafter(po, f32(np.inf)), np.nextafter(po, f32(-np.inf))
    return np.where(off > 0, up, np.where(off < 0, down, po)).astype(f32)


def mirror_step(p, perr, n, ns, dpdu, wo, kr):
    """(rays [m, 7] float32: o, d, tMax = inf, zeros where refused; followed [m] int32)."""
    arrs = [np.ascontiguousarray(a, dtype=f32).reshape(-1, 3) for a in (p, perr, n, ns, dpdu, wo, kr)]
    p, perr, n, ns, dpdu, wo, kr = arrs
    with np.errstate(all="ignore"):
        ss = _normalize(dpdu)
        ts = _cross(ns, ss)
        wl = np.stack([_dot(wo, ss), _dot(wo, ts), _dot(wo, ns)], axis=1)   # to_local
        ok = wl[:, 2] != 0                                                   # wo in the tangent plane: pdf stays 0
        wl = wl * np.asarray([-1, -1, 1], dtype=f32)                         # (-wo.x, -wo.y, wo.z)
        f = (kr / np.abs(wl[:, 2])[:, None]).astype(f32)                     # Kr / |cos|, the no-op Fresnel being 1
        ok &= ~(f == 0).all(axis=1)
        wi = np.stack([((ss[:, c] * wl[:, 0] + ts[:, c] * wl[:, 1]).astype(f32) + ns[:, c] * wl[:, 2]).astype(f32)
                       for c in range(3)], axis=1)                          # to_world
        ok &= np.abs(_dot(wi, ns)) != 0
        o = offset_ray_origin(p, perr, n, wi)
    rays = np.zeros((p.shape[0], 7), dtype=f32)
    rays[ok, 0:3] = o[ok]
    rays[ok, 3:6] = wi[ok]
    rays[ok, 6] = np.inf
    return rays, ok.astype(np.int32)


def step_of_words(words, kr):
    """mirror_step on pbr_hip_query records given as float32 words [m, 28]."""
    return mirror_step(words[:, W_P], words[:, W_PERR], words[:, W_N], words[:, W_NS], words[:, W_DPDU], words[:, W_WO], kr)


def sample_values(query, scene, rd, first, n, bounces, albedo=None, pixels=None, info=None):
    """The eight values of every sample with up to `bounces` mirror steps: float32 [npx, n, 8].
    query: rays [m, 7] → pbr_hip_query records as float32 words [m, 28].  albedo: a function (words, material
    indices) → float32 [m, 3] replacing the materials' constants (textured scenes).  info (a dict) receives per
    sample `steps` (mirror steps taken), `fallback` (a continuation missed and the mirror was kept) and
    `ended_on_mirror` (the recorded surface is a mirror)."""
    rays, _ = E.camera_rays(rd, first, n, pixels)
    m = rays.shape[0]
    mats = E.prim_materials(scene)
    table = [E.material_albedo(mt) for mt in scene.materials]
    const = np.stack([t[0] for t in table]) if table else np.zeros((0, 3), dtype=f32)
    types = np.asarray([mt.type for mt in scene.materials], dtype=np.int64)
    v = np.zeros((m, CH), dtype=f32)
    T = np.zeros(m, dtype=f32)
    steps = np.zeros(m, dtype=np.int64)
    fallback = np.zeros(m, dtype=bool)
    on_mirror = np.zeros(m, dtype=bool)
    active = np.arange(m)
    cur = rays
    while active.size:
        w = np.asarray(query(cur), dtype=f32).reshape(-1, 28)
        hit = w[:, W_HIT].view(np.int32) != 0
        fallback[active[~hit]] = steps[active[~hit]] > 0   # (the record of the mirror it left stays)
        a, w = active[hit], w[hit]
        if not a.size:
            break
        mi = mats[w[:, W_PRIM].view(np.int32).astype(np.int64)]
        assert (mi >= 0).all() and all(table[k][1] for k in set(mi.tolist())), "material-less primitives are not restated"
        alb = const[mi] if albedo is None else np.asarray(albedo(w, mi), dtype=f32).reshape(-1, 3)
        started = v[a, 3] != 0
        v[a, 0:3] = np.where(started[:, None], (v[a, 0:3] * alb).astype(f32), alb)
        v[a, 3] = 1
        v[a, 4:7] = w[:, W_NS]
        T[a] = (T[a] + w[:, W_T]).astype(f32)
        v[a, 7] = T[a]
        mirror = types[mi] == capi.MAT_MIRROR
        on_mirror[a] = mirror
        want = mirror & (steps[a] < bounces)
        nxt, followed = step_of_words(w[want], alb[want])
        go = followed != 0
        active = a[want][go]
        steps[active] += 1
        cur = nxt[go]
    if info is not None:
        info.update(steps=steps.reshape(-1, n), fallback=fallback.reshape(-1, n), ended_on_mirror=on_mirror.reshape(-1, n))
    return v.reshape(-1, n, CH)


def expected(query, scene, rd, first, n, bounces, acc=None, albedo=None, info=None):
    """(accumulator, image) after samples [first, first + n) continue `acc` (None: from zero)."""
    a = E.accumulate(sample_values(query, scene, rd, first, n, bounces, albedo, info=info), acc)
    return a, E.image(a, first + n)
