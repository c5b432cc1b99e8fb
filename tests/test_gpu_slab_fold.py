"""The folded slab test of the quad walks (pbr_slab.h slab_fold; PBR_SLAB_FOLD, PBR_SLAB_FOLD_LANE)
on the rays where it and the reference's sequence could part.

The packet walk tests a wave's foldable rays (finite non-zero 1/d, finite origin) with a three-way
max / min and one comparison, and every other ray — a ±0 or denormal direction component makes 1/d
infinite, and 0·∞ = NaN with the origin on a box plane — with the reference's sequence of comparisons
and selects; a wave that holds both kinds splits, as it does for mixed sign octants.  Which form a lane
runs may not change a bit: every walk must return the oracle's records as uint32 on

  * whole waves of foldable rays of one octant, and of axis-parallel rays (one and two ±0 components);
  * waves with 1, 32 and 63 non-foldable lanes among foldable ones, of one octant and of several;
  * rays with a denormal direction component (1/d infinite, and 1/d finite: 2^-127);
  * origins exactly on planes of the lattice's node boxes, foldable and not;
  * tMax at a node box's entry distance, one ulp either side of it, and infinite;
  * waves with one live lane.

Three scenes: the fixture mesh tests/golden/mesh_small.3d (110 triangles), the 1152-triangle mesh of
the intersect fixture (ref_scenes.intersect_case) and a lattice of 216 axis-aligned triangles on
multiples of ½, whose every box plane is such a multiple.  A caller-built
tree with an inverted box on the rays' way shows that the scene's flag sends the whole scene to the
exact form, and a small frame of the benchmarked shape equals the megakernel's.

Origins on node planes are made for the lattice only.  On the 1152-triangle mesh such an origin lies
in the mesh's seam (x = -1.6e-16) and, with d.x = +0, the ray runs inside it through edges that several
triangles share at the same t.  One such ray (o = (-1.6147258e-16, 1.5356301, 1.0243011), d = (0,
-0.47388965, -0.93073708)) gets primitive 26 from every closest-hit quad walk, with or without this
file's code, where the oracle's binary walk gets 24 at the same t: Triangle::Intersect compares scaled
distances, so a later hit can raise ray.tMax by an ulp (1.1005267 to 1.1005268), and a slot the quad walk
dropped at its node step (tEnter = the old tMax) would have passed when the binary walk reached it.
That is the quad walk's own, older deviation, not a property of the slab test."""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_scenes as RS
from pysicalbasedraytracer_amd import HipRenderer, capi, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
INF = F(np.inf)
TINY = F(1e-39)                 # denormal: 1/TINY overflows to infinity
DENORMAL_FINITE = F(2.0) ** -127   # denormal, 1/d = 2^127 is finite: a foldable ray
SIGNS = [np.array([-1.0 if (o >> a) & 1 else 1.0 for a in range(3)]) for o in range(8)]   # octant: bit a = d[a] < 0


def fixture_mesh():
    P, I = scenes.load_3d(os.path.join(HERE, "golden", "mesh_small.3d"))
    s = scenes.Scene()
    s.mesh(P, I, s.matte((0.5, 0.5, 0.5)))
    return s, P, I


def mesh_1152():
    P, I, _ = RS.small_mesh(24)
    assert len(I) == 1152
    s = scenes.Scene()
    s.mesh(P, I, s.matte((0.5, 0.5, 0.5)))
    return s, P, I


def half_lattice(n=3):
    """Sheets of RS.grid_mesh(n) scaled by ½ at z = 0, ½, .. n/2 and the same sheets turned to the x
    and y planes: 3 (n + 1) meshes of 2 n² triangles, every coordinate a multiple of ½."""
    s = scenes.Scene()
    m = s.matte((0.5, 0.5, 0.5))
    P, I = RS.grid_mesh(n)
    Ps, Is = [], []
    for k in range(n + 1):
        Q = ((P + F([0, 0, k])) * F(0.5)).astype(F)
        for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
            s.mesh(Q[:, perm].copy(), I, m)
            Is.append(I + sum(len(p) for p in Ps))
            Ps.append(Q[:, perm])
    return s, np.concatenate(Ps), np.concatenate(Is)


def node_boxes(scene):
    """(lo [n, 3], hi [n, 3]) of every node of the tree the upload builds (the oracle's is that tree)."""
    raw, _ = O.build_bvh(scene)
    L = raw.view(np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("offset", "<i4"), ("n", "<u2"), ("axis", "u1"), ("pad", "u1")]))
    return L["lo"].copy(), L["hi"].copy()


def entry_distance(lo, hi, o, d):
    """The reference's slab sequence in float32, one operation at a time, per row: (passes whatever
    ray.tMax is, tMin)."""
    with np.errstate(all="ignore"):
        inv = F(1) / d
        neg = inv < 0
        nr, fr = np.where(neg, hi, lo), np.where(neg, lo, hi)
        tn, tf = ((nr - o) * inv).astype(F), ((fr - o) * inv).astype(F)
        tMin, tMax = tn[:, 0], tf[:, 0]
        ok = ~(tMin > tf[:, 1]) & ~(tn[:, 1] > tMax)
        tMin = np.where(tn[:, 1] > tMin, tn[:, 1], tMin)
        tMax = np.where(tf[:, 1] < tMax, tf[:, 1], tMax)
        ok &= ~(tMin > tf[:, 2]) & ~(tn[:, 2] > tMax)
        tMin = np.where(tn[:, 2] > tMin, tn[:, 2], tMin)
        tMax = np.where(tf[:, 2] < tMax, tf[:, 2], tMax)
        return ok & (tMax > 0), tMin


def forms_part(lo, hi, rays):
    """Per ray: the number of node boxes (lo, hi: [n, 3]) that the reference's sequence and the folded
    form (fmax / fmin drop a NaN, one comparison of the extremes) decide differently, ray.tMax aside."""
    out = np.zeros(len(rays), int)
    n = len(lo)
    with np.errstate(all="ignore"):
        for i, r in enumerate(rays):
            o, d = np.tile(r[:3], (n, 1)), np.tile(r[3:6], (n, 1))
            exact, _ = entry_distance(lo, hi, o, d)
            inv = F(1) / d
            neg = inv < 0
            tn = ((np.where(neg, hi, lo) - o) * inv).astype(F)
            tf = ((np.where(neg, lo, hi) - o) * inv).astype(F)
            tmin = np.fmax(np.fmax(tn[:, 0], tn[:, 1]), tn[:, 2])
            tmax = np.fmin(np.fmin(tf[:, 0], tf[:, 1]), tf[:, 2])
            out[i] = int((exact != (~(tmin > tmax) & (tmax > 0))).sum())
    return out


def foldable(rays):
    with np.errstate(all="ignore"):
        inv = F(1) / rays[:, 3:6]
    return np.isfinite(inv).all(1) & (inv != 0).all(1) & np.isfinite(rays[:, :3]).all(1)


def dead(n):
    """Lanes that fail the root test: far outside, ending at once."""
    return np.tile(F([-1000, -1000, -1000, 1, 1, 1, 0]), (n, 1))


class Maker:
    """Seeded rays aimed at the triangles of (P, I)."""

    def __init__(self, P, I, seed):
        self.P, self.I = P.astype(np.float64), I
        self.rng = np.random.default_rng(seed)
        self.size = float((P.max(0) - P.min(0)).max())

    def targets(self, n):
        tri = self.P[self.I[self.rng.integers(0, len(self.I), n)]]
        w = self.rng.dirichlet((1.0, 1.0, 1.0), n)
        return (w[:, :, None] * tri).sum(1)

    def octant(self, n, octant):
        """Foldable rays of one sign octant, from 0.2 to 1.2 sizes away."""
        t = self.targets(n)
        d = self.rng.uniform(0.2, 1.0, (n, 3)) * SIGNS[octant]
        k = self.rng.uniform(0.2, 1.2, (n, 1)) * self.size
        return np.concatenate([t - d * k, d, np.full((n, 1), np.inf)], 1).astype(F)

    def axis_parallel(self, n, zeros, octant):
        """`zeros` direction components ±0 (both signs), the others of the octant; the origin moved
        off the target along the non-zero components only, so the ray still passes through it."""
        r = self.octant(n, octant).astype(np.float64)
        tgt = self.targets(n)
        for i in range(n):
            ax = self.rng.permutation(3)[:zeros]
            d = r[i, 3:6].copy()
            d[ax] = self.rng.choice([0.0, -0.0], zeros)
            r[i, 3:6] = d
            r[i, :3] = tgt[i] - d * self.rng.uniform(0.2, 1.2) * self.size
        return r.astype(F)

    def tiny(self, n, octant, value):
        """One direction component ±value, the origin on the target's coordinate of that axis."""
        r = self.octant(n, octant).astype(np.float64)
        tgt = self.targets(n)
        for i in range(n):
            a = self.rng.integers(3)
            d = r[i, 3:6].copy()
            d[a] = float(value) * self.rng.choice([-1.0, 1.0])
            r[i, 3:6] = d
            o = tgt[i] - d * self.rng.uniform(0.2, 1.2) * self.size
            o[a] = tgt[i][a]
            r[i, :3] = o
        return r.astype(F)


def mixed_wave(mk, n_bad, octants):
    """64 lanes: n_bad non-foldable ones (±0 and denormal components) at seeded positions among
    foldable ones of `octants`."""
    lanes = np.concatenate([mk.octant(1, octants[i % len(octants)]) for i in range(64)])
    where = mk.rng.permutation(64)[:n_bad]
    for j, i in enumerate(where):
        o = octants[i % len(octants)]
        lanes[i] = (mk.axis_parallel(1, 1 + j % 2, o) if j % 3 else mk.tiny(1, o, TINY))[0]
    assert (~foldable(lanes)).sum() == n_bad
    return lanes


def on_planes(mk, lo, hi, n):
    """Origins exactly on a plane of a node box (one axis), half of them with that direction
    component ±0 (the ray slides along the plane: 0·∞ = NaN there), half foldable."""
    planes = [np.unique(np.concatenate([lo[:, a], hi[:, a]])) for a in range(3)]
    r = np.concatenate([mk.octant(1, int(mk.rng.integers(8))) for _ in range(n)])
    for i in range(n):
        a = int(mk.rng.integers(3))
        r[i, a] = mk.rng.choice(planes[a])
        if i % 2:
            r[i, 3 + a] = mk.rng.choice([0.0, -0.0])
    return r


def tmax_at_entries(mk, lo, hi, n):
    """Foldable rays ending at the entry distance of a node box they pass, one ulp either side of it,
    and not at all: four rays each."""
    base = np.concatenate([mk.octant(1, int(mk.rng.integers(8))) for _ in range(n)])
    out = []
    for r in base:
        ok, t = entry_distance(lo, hi, np.tile(r[:3], (len(lo), 1)), np.tile(r[3:6], (len(lo), 1)))
        cand = np.nonzero(ok & (t > 0) & np.isfinite(t))[0]
        if len(cand) == 0:
            continue
        te = t[mk.rng.choice(cand)]
        for tm in (te, np.nextafter(te, INF), np.nextafter(te, F(0)), INF):
            q = r.copy()
            q[6] = tm
            out.append(q)
    return np.array(out, F)


def make_rays(P, I, lo, hi, seed, planes):
    """{class: rays}; every class a whole number of 64-ray waves (padded with dead lanes).  planes:
    with the origins on node planes (the lattice)."""
    mk = Maker(P, I, seed)

    def waves(r):
        return np.concatenate([r, dead(-len(r) % 64)])

    c = {}
    c["octant"] = np.concatenate([mk.octant(128, o) for o in range(8)])
    c["axis1"] = np.concatenate([mk.axis_parallel(64, 1, o) for o in range(8)])
    c["axis2"] = np.concatenate([mk.axis_parallel(64, 2, o) for o in range(8)])
    c["mixed_one_octant"] = np.concatenate([mixed_wave(mk, nb, [o]) for nb in (1, 32, 63) for o in (0, 5, 7)])
    c["mixed_octants"] = np.concatenate([mixed_wave(mk, nb, octs) for nb in (1, 32, 63) for octs in ([0, 7], [1, 2, 4], list(range(8)))])
    c["denormal"] = waves(np.concatenate([mk.tiny(48, o, v) for o in (0, 3, 6) for v in (TINY, DENORMAL_FINITE)]))
    if planes:
        c["on_planes"] = waves(on_planes(mk, lo, hi, 768))
    c["tmax_entry"] = waves(tmax_at_entries(mk, lo, hi, 256))
    lone = []
    for lane in (0, 31, 63):
        for kind in range(3):
            w = dead(64)
            w[lane] = (mk.octant(1, lane % 8), mk.axis_parallel(1, 1, lane % 8), mk.tiny(1, lane % 8, TINY))[kind][0]
            lone.append(w)
    c["lone_lane"] = np.concatenate(lone)
    return c


SCENES = {"fixture_mesh": fixture_mesh, "mesh_1152": mesh_1152, "lattice": half_lattice}
_cases = {}


def case(name):
    """name → (scene, rays, [(class, count)], closest records, any-hit records, classes dict)."""
    if name not in _cases:
        s, P, I = SCENES[name]()
        lo, hi = node_boxes(s)
        cls = make_rays(P, I, lo, hi, 31 + list(SCENES).index(name), planes=name == "lattice")
        rays = np.concatenate(list(cls.values()))
        _cases[name] = (s, rays, [(k, len(v)) for k, v in cls.items()], O.intersect(s, rays, any_hit=False),
                        O.intersect(s, rays, any_hit=True), cls)
    return _cases[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_the_rays_are_what_the_docstring_says(name):
    s, rays, classes, want, want_any, cls = case(name)
    assert 4000 <= len(rays) <= 9000 and len(rays) % 64 == 0
    assert all(len(v) % 64 == 0 for v in cls.values())
    assert foldable(cls["octant"]).all()
    assert not foldable(cls["axis1"]).any() and not foldable(cls["axis2"]).any()
    assert ((cls["axis1"][:, 3:6] == 0).sum(1) == 1).all() and ((cls["axis2"][:, 3:6] == 0).sum(1) == 2).all()
    for k in ("axis1", "axis2"):
        z = cls[k][:, 3:6]
        assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()   # both signs of zero
    bad = [(~foldable(w)).sum() for k in ("mixed_one_octant", "mixed_octants") for w in cls[k].reshape(-1, 64, 7)]
    assert sorted(set(bad)) == [1, 32, 63]
    live = cls["denormal"][cls["denormal"][:, 6] > 0]
    tiny = np.abs(live[:, 3:6]) < F(1.2e-38)
    assert (tiny.sum(1) == 1).all() and 0 < foldable(live).sum() < len(live)   # 1/d infinite, and 2^127
    assert ("on_planes" in cls) == (name == "lattice")
    if "on_planes" in cls:
        lo, hi = node_boxes(s)
        p = cls["on_planes"][:768]
        on = np.zeros(len(p), bool)
        for a in range(3):
            on |= np.isin(p[:, a], np.concatenate([lo[:, a], hi[:, a]]))
        assert on.all() and 0 < foldable(p).sum() < len(p)
        assert (p[:, :3] % 0.5 == 0).any(1).all()   # the lattice's planes are multiples of ½
    te = cls["tmax_entry"]
    assert len(te) >= 512 and np.isfinite(te[:, 6]).sum() >= 384
    for w in cls["lone_lane"].reshape(-1, 64, 7):
        assert (w[:, 6] > 0).sum() == 1
    # Where the forms part: on no box of the tree for a foldable ray; for the non-foldable classes on
    # boxes of the tree itself, so a walk that folded those lanes would test differently
    lo, hi = node_boxes(s)
    live = rays[:, 6] > 0
    fo = foldable(rays) & live
    assert forms_part(lo, hi, rays[fo][::8]).sum() == 0
    parted = {k: forms_part(lo, hi, cls[k][~foldable(cls[k]) & (cls[k][:, 6] > 0)]) for k in ("axis1", "axis2", "on_planes") if k in cls}
    print(name, {k: f"{int((v > 0).sum())} of {len(v)} rays, {int(v.sum())} boxes" for k, v in parted.items()})
    # The forms part only on a NaN: an infinite 1/d alone gives ±inf, which both treat alike.  A mesh's
    # axis-parallel rays meet a box plane exactly only by chance; the lattice's on-plane rays with that
    # component ±0 do on every box with that plane, and the reference's sequence keeps a NaN only from
    # the x axis (tMin and tMax start there), so about a third of them part: at least a sixth must.
    if name == "lattice":
        assert (parted["on_planes"] > 0).sum() * 6 >= len(parted["on_planes"])
    # the walks have something to find: hits and misses in every class but the dead padding
    edges = np.cumsum([0] + [n for _, n in classes])
    for (k, n), a, b in zip(classes, edges[:-1], edges[1:]):
        h = want[a:b, 0] > 0
        print(f"{name} {k}: {n} rays, {int(h.sum())} hit, {int(foldable(rays[a:b]).sum())} foldable")
        assert h.any(), k
    assert 0.3 < (want[:, 0] > 0).mean() < 0.98
    assert (want_any[:, 0] > 0).sum() == (want[:, 0] > 0).sum()


@pytest.fixture(scope="module")
def hip():
    h = HipRenderer(0)
    yield h
    h.close()


# (id, walk, any hit, extra): the packet walk has no any-hit entry
WALKS = [
    ("packet-closest", capi.WALK_PACKET, False, {}),
    ("packet_queue-closest", capi.WALK_PACKET, False, {"seg_cap": 64}),
    ("lane-closest", capi.WALK_LANE, False, {}),
    ("lane-any", capi.WALK_LANE, True, {}),
    ("lane_lds-closest", capi.WALK_LANE_LDS, False, {}),
    ("lane_lds-any", capi.WALK_LANE_LDS, True, {}),
    ("refill-closest", capi.WALK_REFILL, False, {}),
    ("refill-any", capi.WALK_REFILL, True, {}),
]


def assert_records(got, want, what, rays, classes=None):
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    if len(bad) == 0:
        return
    where = ""
    if classes:
        edges = np.cumsum([0] + [n for _, n in classes])
        where = f" by class { {k: int(((bad >= a) & (bad < b)).sum()) for (k, _), a, b in zip(classes, edges[:-1], edges[1:])} };"
    first = "; ".join(f"ray {i} {rays[i].tolist()}: got {got[i].tolist()} want {want[i].tolist()}" for i in bad[:4])
    raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ from the oracle's;{where} {first}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_walks_equal_the_oracle(hip, name):
    s, rays, classes, want, want_any, cls = case(name)
    hip.upload(s)
    for walk_id, walk, any_hit, extra in WALKS:
        got = hip.intersect_walk(rays, walk, any_hit=any_hit, **extra)
        assert_records(got, want_any if any_hit else want, f"{walk_id} on {name}", rays, classes)


def inverted_tree():
    """The lattice with its primitives in leaf order and its own tree handed over, one interior box
    two levels below the root (a slot of the root quad node) inverted on x: its planes put an eighth
    either side of the middle of its extent, the upper one first.
    Returns (scene, the box's node index, lo and hi of the inverted box, the slots of the primitives
    below it, the mesh in leaf order)."""
    s, P, I = half_lattice()
    cn, ci = O.build_bvh(s)
    rec = np.frombuffer(cn.tobytes(), dtype=[("lo", "<f4", 3), ("hi", "<f4", 3), ("off", "<i4"), ("np", "<u2"), ("ax", "u1"), ("pad", "u1")])
    child = 1 if rec["np"][1] == 0 else int(rec["off"][0])
    assert rec["np"][child] == 0
    k = child + 1 if rec["np"][child + 1] == 0 else int(rec["off"][child])
    assert rec["np"][k] == 0 and rec["lo"][k][0] < rec["hi"][k][0]
    bad = cn.copy().view(F).reshape(-1, 8)
    mid = F(0.5) * (bad[k, 0] + bad[k, 3])
    bad[k, 0], bad[k, 3] = mid + F(0.125), mid - F(0.125)
    lo, hi = bad[k, :3].copy(), bad[k, 3:6].copy()
    t = scenes.Scene()
    t.mesh(P, np.ascontiguousarray(I[ci]), t.matte((0.5, 0.5, 0.5)))
    t.bvh_nodes = bad.view(np.uint8).reshape(-1)
    below, todo = [], [k]
    while todo:
        i = todo.pop()
        if rec["np"][i] > 0:
            below += range(int(rec["off"][i]), int(rec["off"][i]) + int(rec["np"][i]))
        else:
            todo += [i + 1, int(rec["off"][i])]
    return t, k, lo, hi, np.array(sorted(below)), P, np.ascontiguousarray(I[ci])


_inverted = []


def inverted_case():
    if not _inverted:
        t, k, lo, hi, below, P, I = inverted_tree()
        mk, aimed = Maker(P, I, 33), Maker(P, I[below], 34)   # at the whole lattice, and at the primitives below the box
        rays = np.concatenate([m.octant(96, o) for o in range(8) for m in (mk, aimed)])
        _inverted.append((t, k, lo, hi, below, rays, O.intersect(t, rays, any_hit=False)))
    return _inverted[0]


def test_the_inverted_box_decides():
    """The reference's sequence never compares an axis' near value with its own far value, so it lets
    rays into the inverted box; the folded form (max of the near values against min of the far ones)
    rejects them.  The primitives below that box are reached through it alone, and the oracle hits
    some of them: a walk that folded in this scene would lose those records."""
    t, k, lo, hi, below, rays, want = inverted_case()
    assert foldable(rays).all()
    behind = (want[:, 0] > 0) & np.isin(want[:, 2].astype(int), below)
    r = rays[behind]
    n = len(r)
    assert n >= 20, n
    assert lo[0] > hi[0]
    inv_lo, inv_hi = lo, hi
    ok, _ = entry_distance(np.tile(inv_lo, (n, 1)), np.tile(inv_hi, (n, 1)), r[:, :3], r[:, 3:6])
    assert ok.all()                                 # the exact sequence let every one of them in
    inv = F(1) / r[:, 3:6]
    neg = inv < 0
    tn = ((np.where(neg, inv_hi, inv_lo) - r[:, :3]) * inv).astype(F)
    tf = ((np.where(neg, inv_lo, inv_hi) - r[:, :3]) * inv).astype(F)
    folded = ~(tn.max(1) > tf.min(1))
    print(f"inverted node {k}: {n} of {len(rays)} rays hit a primitive below it; the folded form would let {int(folded.sum())} in")
    assert (~folded).sum() >= 20


@pytest.mark.gpu
def test_an_inverted_box_sends_the_scene_to_the_exact_form(hip):
    t, k, lo, hi, below, rays, want = inverted_case()
    hip.upload(t)
    for walk_id, walk, any_hit, extra in WALKS:
        if any_hit:
            continue
        got = hip.intersect_walk(rays, walk, any_hit=False, **extra)
        assert_records(got, want, f"{walk_id} on the tree with an inverted box", rays)


@pytest.mark.gpu
def test_a_c2_shaped_frame_equals_the_megakernels(hip):
    """64 spp (a wave is one pixel's samples), a mirror floor, 288 triangles: the wavefront frame,
    whose level 0 walks packets, against the same library's megakernel frame, which walks per lane."""
    P, I = scenes.dragon_standin(n=12)
    assert len(I) == 288
    s, rd = scenes.config_c2(96, 54, 64, mesh=(P, I, "standin-12"), sky=scenes.procedural_sky(128, 64))
    hip.upload(s)
    hip.set_schedule(kernels=capi.KERNELS_MEGAKERNEL)
    mk, mk8, _ = hip.render(rd)
    assert hip.last_chunks()["n_chunks"] == 0
    hip.set_schedule()
    g, g8, _ = hip.render(rd)
    assert hip.last_chunks()["n_chunks"] >= 1
    assert np.any(mk != 0)
    diff = (g.view(np.uint32) != mk.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {len(diff)} float pixels differ from the megakernel's"
    assert np.array_equal(g8, mk8)
