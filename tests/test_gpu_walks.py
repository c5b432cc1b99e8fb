"""Every production BVH walk on caller-given rays, against the oracle and the reference's records.

pbr_hip_intersect runs the per-lane quad walk with a private stack; a rendered frame spends its
time in other walks — the LDS short stack, the wave packet, lane refill over a segmented queue, the
binary walk of deep trees — which whole renders pin only on the rays a camera or a BSDF produces.
pbr_hip_intersect_walk sends caller rays through each of them with the template arguments and
launch bounds of its production users, and here every walk and hit mode must return
the oracle's records bit for bit (hit, t, primitive, b1, b2 as uint32) on the rays renders never
see: ±0 direction components with origins on box planes (0·inf = NaN in the slab test), all eight
sign octants in one wave, tMax at the hit distance and one ulp either side, waves with one live
lane, trees from empty to one leaf to a few nodes, and queues whose segment counts no shade kernel
would write (tests/ref_scenes.py walk_case(); tests/test_walk_fixtures.py pins the expected values
to the reference on the CPU)."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import ref_scenes as RS
from pysicalbasedraytracer_amd import HipRenderer, capi
from test_ref_fixtures import intersect_fixture
from test_stack_depth import chain_rays, deep_scene

pytestmark = pytest.mark.gpu

# (id, walk, any_hit, extra arguments) — every walk x mode with a production user; the packet walk
# has no any-hit user (traverse_wave<true> is instantiated nowhere) and the transmittance kernel's
# lane refill no closest-hit one
WALKS = [
    ("lane-closest", capi.WALK_LANE, False, {}),
    ("lane-any", capi.WALK_LANE, True, {}),
    ("lane_lds-closest", capi.WALK_LANE_LDS, False, {}),
    ("lane_lds-any", capi.WALK_LANE_LDS, True, {}),
    ("packet-closest", capi.WALK_PACKET, False, {}),
    ("packet_queue-closest", capi.WALK_PACKET, False, {"seg_cap": 64}),
    ("refill-closest", capi.WALK_REFILL, False, {}),
    ("refill-any", capi.WALK_REFILL, True, {}),
    ("refill_tr-any", capi.WALK_REFILL_TR, True, {}),
    ("binary-closest", capi.WALK_BINARY, False, {}),
    ("binary-any", capi.WALK_BINARY, True, {}),
]
WALK_IDS = [w[0] for w in WALKS]
QUEUE_WALKS = [w for w in WALKS if w[0] in ("packet_queue-closest", "refill-closest", "refill-any", "refill_tr-any")]


def lattice():
    s, rays, classes = RS.walk_fixture_rays()
    return s, rays


def intersect_1152():
    return RS.intersect_case()


SCENES = {"lattice": lattice, "intersect_1152": intersect_1152}
for _name in RS.walk_small_scenes():
    SCENES[_name] = (lambda n: lambda: RS.walk_small_scenes()[n])(_name)


class State:
    """One renderer; the scene on the device, the oracle's and pbr_hip_intersect's records per scene."""

    def __init__(self):
        self.hip = HipRenderer(0)
        self.name = None
        self.cases = {}
        self.want = {}
        self.base = {}

    def use(self, name, make):
        if name not in self.cases:
            self.cases[name] = make()
        s, rays = self.cases[name]
        if self.name != name:
            self.hip.upload(s)
            self.name = name
        return s, rays

    def oracle(self, name, any_hit):
        if (name, any_hit) not in self.want:
            s, rays = self.cases[name]
            self.want[name, any_hit] = O.intersect(s, rays, any_hit=any_hit)
        return self.want[name, any_hit]

    def baseline(self, name, any_hit):
        if (name, any_hit) not in self.base:
            assert self.name == name
            self.base[name, any_hit] = self.hip.intersect(self.cases[name][1], any_hit=any_hit)
        return self.base[name, any_hit]


@pytest.fixture(scope="module")
def st():
    s = State()
    yield s
    s.hip.close()


def assert_records(got, want, what, rays, classes=None):
    """All five floats of every record as uint32; a failure names the ray classes and first rays."""
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    if len(bad) == 0:
        return
    where = ""
    if classes:
        edges = np.cumsum([0] + [c[1] for c in classes])
        per = {c[0]: int(((bad >= lo) & (bad < hi)).sum()) for c, lo, hi in zip(classes, edges[:-1], edges[1:])}
        where = f" by class {per};"
    first = "; ".join(f"ray {i} {rays[i].tolist()}: got {got[i].tolist()} want {want[i].tolist()}" for i in bad[:4])
    raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ;{where} {first}")


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("walk_id,walk,any_hit,extra", WALKS, ids=WALK_IDS)
def test_walk_equals_oracle(st, scene, walk_id, walk, any_hit, extra):
    s, rays = st.use(scene, SCENES[scene])
    classes = RS.walk_fixture_rays()[2] if scene == "lattice" else None
    got = st.hip.intersect_walk(rays, walk, any_hit=any_hit, **extra)
    assert_records(got, st.oracle(scene, any_hit), f"{walk_id} on {scene} vs the oracle", rays, classes)
    assert_records(got, st.baseline(scene, any_hit), f"{walk_id} on {scene} vs pbr_hip_intersect", rays, classes)


@pytest.mark.parametrize("walk_id,walk,any_hit,extra", WALKS, ids=WALK_IDS)
def test_walk_wave_shapes(st, walk_id, walk, any_hit, extra):
    """n = 1, 63, 64, 65, 129 and waves whose only live lane is lane 0, 31 or 63."""
    s, _ = st.use("lattice", SCENES["lattice"])
    for name, rays in RS.walk_wave_shapes().items():
        if ("shape", name, any_hit) not in st.want:
            st.want["shape", name, any_hit] = O.intersect(s, rays, any_hit=any_hit)
        got = st.hip.intersect_walk(rays, walk, any_hit=any_hit, **extra)
        assert_records(got, st.want["shape", name, any_hit], f"{walk_id}, wave shape {name}", rays)
        assert_records(got, st.hip.intersect(rays, any_hit=any_hit), f"{walk_id}, wave shape {name} vs pbr_hip_intersect", rays)


LAYOUTS = RS.walk_seg_layouts()


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("walk_id,walk,any_hit,extra", QUEUE_WALKS, ids=[w[0] for w in QUEUE_WALKS])
def test_queue_walk_segment_layouts(st, layout, walk_id, walk, any_hit, extra):
    """The same records in the same ray order whatever the queue's segment counts."""
    name, n, cap, counts = layout
    s, _ = st.use("lattice", SCENES["lattice"])
    rays = RS.walk_mixed(n)
    if ("mixed", any_hit) not in st.want:
        st.want["mixed", any_hit] = O.intersect(s, RS.walk_mixed(), any_hit=any_hit)
    got = st.hip.intersect_walk(rays, walk, any_hit=any_hit, seg_counts=counts, seg_cap=cap)
    assert_records(got, st.want["mixed", any_hit][:n], f"{walk_id}, layout {name}", rays)


def check_closest(got, ref):
    """test_ref_fixtures.check_hits, the closest-hit part: the reference records hit, t, primitive."""
    hit = ref[:, 0] == 1
    assert np.array_equal(got[:, 0] == 1, hit)
    assert np.array_equal(got[hit, 1].view(np.uint32), ref[hit, 1].view(np.uint32)), "hit distances differ"
    assert np.array_equal(got[hit, 2], ref[hit, 2]), "hit primitives differ"


@pytest.mark.parametrize("fixture", ["walk_rays", "intersect"])
@pytest.mark.parametrize("walk_id,walk,any_hit,extra", WALKS, ids=WALK_IDS)
def test_walk_equals_reference_records(st, fixture, walk_id, walk, any_hit, extra):
    """Against the reference's own records: tests/golden/walk_rays.json (the lattice rays) and the
    `intersect` fixture of ref_fixtures.json."""
    if fixture == "walk_rays":
        s, rays = st.use("lattice", SCENES["lattice"])
        ref, anyref, f = RS.load_walk_fixture()
        assert f["scene_digest"] == RS.scene_digest(s)
        assert f["rays_sha256"] == hashlib.sha256(rays.astype("<f4").tobytes()).hexdigest()
    else:
        s, rays = st.use("intersect_1152", SCENES["intersect_1152"])
        _, rays2, ref, anyref = intersect_fixture()
        assert np.array_equal(rays.view(np.uint32), rays2.view(np.uint32))
    got = st.hip.intersect_walk(rays, walk, any_hit=any_hit, **extra)
    if any_hit:
        assert np.array_equal(got[:, 0] == 1, anyref == 1)
    else:
        check_closest(got, ref)


def walk_rc(hip, walk, rays, any_hit=0, seg_cap=0, counts=None, n=None):
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
    out = np.empty((max(len(r), 1), 5), np.float32)
    c = None if counts is None else np.ascontiguousarray(counts, np.int32)
    return hip.lib.pbr_hip_intersect_walk(hip.ctx, walk, len(r) if n is None else n, capi.fptr(r), capi.fptr(out), any_hit, seg_cap,
                                          None if c is None else capi.iptr(c))


def test_deep_tree_walks_and_refusals(st):
    """The 47-level chain mesh (quad stack need 69 > 61: walked in binary form): LANE and BINARY
    equal the oracle; every quad, packet and refill walk is refused — the entry must not walk a
    quad tree its stack cannot hold.  And the argument checks of the entry."""
    hip = st.hip
    s = deep_scene()
    hip.upload(s)
    st.name = None
    rays = chain_rays(3000, 3)
    for any_hit in (False, True):
        want = O.intersect(s, rays, any_hit=any_hit)
        for walk in (capi.WALK_LANE, capi.WALK_BINARY):
            assert_records(hip.intersect_walk(rays, walk, any_hit=any_hit), want, f"walk {walk} on the chain mesh", rays)
    assert (want[:, 0] > 0).mean() > 0.2
    for walk, any_hit, cap in ((capi.WALK_LANE_LDS, 0, 0), (capi.WALK_LANE_LDS, 1, 0), (capi.WALK_PACKET, 0, 0), (capi.WALK_PACKET, 0, 64),
                               (capi.WALK_REFILL, 0, 0), (capi.WALK_REFILL, 1, 0), (capi.WALK_REFILL_TR, 1, 0)):
        assert walk_rc(hip, walk, rays, any_hit, cap) == capi.PBR_E_UNSUPPORTED, (walk, any_hit)
    with pytest.raises(RuntimeError, match="binary form"):
        hip.intersect_walk(rays, capi.WALK_REFILL)

    s, rays = st.use("lattice", SCENES["lattice"])
    rays = rays[:100]
    S = capi.WALK_SEGMENTS
    for walk in (-1, 6, 99):
        assert walk_rc(hip, walk, rays) == capi.PBR_E_INVALID
    good = np.zeros(S, np.int32)
    good[5], good[S - 1] = 60, 40
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, 64, good) == capi.PBR_OK
    short = good.copy()
    short[5] = 59
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, 64, short) == capi.PBR_E_INVALID          # sums to n - 1
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, 50, good) == capi.PBR_E_INVALID           # an entry above seg_cap
    neg = good.copy()
    neg[5], neg[6] = 61, -1
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, 64, neg) == capi.PBR_E_INVALID
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, (256 << 20) // (48 * S) + 1) == capi.PBR_E_INVALID   # queue above 256 MB
    assert walk_rc(hip, capi.WALK_REFILL, rays, 0, -1) == capi.PBR_E_INVALID
    assert walk_rc(hip, capi.WALK_REFILL, np.tile(rays, (30, 1)), 0, 1) == capi.PBR_E_INVALID   # more rays than the queue holds
    assert walk_rc(hip, capi.WALK_LANE, rays, 0, 64) == capi.PBR_E_INVALID                   # a walk that reads no queue
    assert walk_rc(hip, capi.WALK_BINARY, rays, 0, 0, good) == capi.PBR_E_INVALID
    assert walk_rc(hip, capi.WALK_PACKET, rays, 1) == capi.PBR_E_UNSUPPORTED                 # no any-hit packet walk
    assert walk_rc(hip, capi.WALK_REFILL_TR, rays, 0) == capi.PBR_E_UNSUPPORTED              # no closest-hit transmittance walk
    for walk in range(6):
        assert walk_rc(hip, walk, rays, 1 if walk == capi.WALK_REFILL_TR else 0, n=0) == capi.PBR_OK   # n = 0: nothing runs
    # the context is still usable; seg_cap = 0 takes the fullest segment's count
    one = np.zeros(S, np.int32)
    one[77] = 100
    got = hip.intersect_walk(rays, capi.WALK_REFILL, seg_counts=one)
    assert_records(got, st.oracle("lattice", False)[:100], "refill, 100 rays in one segment, seg_cap = 0", rays)
    got = hip.intersect_walk(rays, capi.WALK_REFILL)
    assert_records(got, st.oracle("lattice", False)[:100], "refill after the refusals", rays)
