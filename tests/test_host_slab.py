"""The quad walks' slab test (pysicalbasedraytracer_amd/csrc/pbr_slab.h) compiled for the host
(tests/cpp_slab/slab_test.cpp): the reference's sequence of comparisons and selects against the folded
form (three-way max and min, one comparison), and the two predicates that decide where the folded form
may run.

  * On foldable rays (finite non-zero 1/d, finite origin) against ordered finite boxes the two forms
    decide alike and give the same tMin, over a seeded set that by itself accepts and rejects at every
    stage often enough to mean something.
  * On rays outside that class the forms do differ: the guard is needed.
  * slab_ray_foldable and slab_scene_foldable return what the statements of them below return.

The program is built twice, plain and with the address and undefined-behaviour sanitizers, and both are
run as programs of their own."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "cpp_slab")
N_EQUAL = 1_000_000


@pytest.fixture(scope="module")
def programs():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "slab_test"), os.path.join(DIR, "slab_test_san")


def run(path, *args):
    p = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr == "", p.stderr[-2000:]   # a sanitizer report
    return p.stdout


def counts(line):
    w = line.split()
    return {k: int(v) for k, v in zip(w[0::2], w[1::2])}


def test_forms_agree_on_foldable_rays(programs):
    out = run(programs[0], "equal", N_EQUAL, 20261021)
    c = counts(out)
    print(c)
    assert c["cases"] == N_EQUAL
    assert c["diff_decision"] == 0 and c["diff_predicate"] == 0
    assert c["diff_tmin"] == 0 and c["diff_tmin_accepted"] == 0 and c["diff_tmax"] == 0   # as numbers (==): ±0 agree
    # the generator meets these shares by itself
    assert c["accept"] >= N_EQUAL // 100
    for stage in ("stage1", "stage2", "stage3", "stage4"):   # the first of the four rejections that fires
        assert c[stage] >= N_EQUAL // 100, stage
    assert c["behind"] >= N_EQUAL // 1000 and c["beyond"] >= N_EQUAL // 1000   # tMax > 0 and tMin < ray.tMax decide too
    assert c["resampled"] < N_EQUAL // 10   # the restriction to foldable pairs removes little
    assert run(programs[1], "equal", N_EQUAL, 20261021) == out


def test_forms_differ_outside_the_class(programs):
    out = run(programs[0], "guard", 100_000, 7)
    rows = {line.split()[0]: counts(line.split(None, 1)[1]) for line in out.splitlines()}
    print(rows)
    assert set(rows) == {"zero", "denormal", "on_plane"}
    for name, c in rows.items():
        assert c["foldable"] == 0, name        # the predicate sends every one of them to the exact form
    assert sum(c["differ"] for c in rows.values()) >= 1
    assert rows["on_plane"]["nan"] >= 1 and rows["on_plane"]["differ"] >= 1   # 0·∞ = NaN decides differently
    assert run(programs[1], "guard", 100_000, 7) == out


def ray_foldable(o, inv):
    """Every 1/d component finite and not zero, every origin component finite."""
    return bool(np.isfinite(inv).all() and (inv != 0).all() and np.isfinite(o).all())


def scene_foldable(quad):
    """Every valid slot of every quad node: six finite planes, lo <= hi on each axis."""
    for w in quad.reshape(-1, 32):
        meta = int(w[28:29].view(np.uint32)[0])
        for s in range(4):
            if not (meta >> (8 + s)) & 1:
                continue
            lo, hi = w[[s, 4 + s, 8 + s]], w[[12 + s, 16 + s, 20 + s]]
            if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
                return False
    return True


def quad_node(boxes, valid):
    """One quad node: boxes = four (lo[3], hi[3]), valid = the slots' mask."""
    w = np.zeros(32, np.float32)
    for s, (lo, hi) in enumerate(boxes):
        w[[s, 4 + s, 8 + s]] = lo
        w[[12 + s, 16 + s, 20 + s]] = hi
    w[28:29].view(np.uint32)[0] = 0 | 1 << 2 | 2 << 4 | valid << 8
    return w


def test_predicates_match_their_statements(programs, tmp_path):
    with np.errstate(divide="ignore", over="ignore"):
        tiny = np.float32(1e-39)
        specials = np.array([0.0, -0.0, tiny, -tiny, np.float32(2.0) ** -127, 1e-30, -1e-30, 1.0, -0.5, 3e38, np.inf, -np.inf, np.nan], np.float32)
        rng = np.random.default_rng(5)
        rows = []
        for d0 in specials:                       # each special in each direction slot, and as an origin
            for a in range(3):
                d = np.array([1.0, -0.5, 0.25], np.float32)
                d[a] = d0
                rows.append(np.concatenate([np.array([1, 2, 3], np.float32), np.float32(1) / d]))
                o = np.array([1, 2, 3], np.float32)
                o[a] = d0
                rows.append(np.concatenate([o, np.array([1.0, -2.0, 4.0], np.float32)]))
        for _ in range(2000):
            d = np.where(rng.random(3) < 0.2, rng.choice(specials, 3), rng.standard_normal(3)).astype(np.float32)
            o = np.where(rng.random(3) < 0.1, rng.choice(specials, 3), rng.standard_normal(3) * 10).astype(np.float32)
            rows.append(np.concatenate([o, np.float32(1) / d]))
    rays = np.array(rows, np.float32)
    want = [ray_foldable(r[:3], r[3:]) for r in rays]
    assert 0.2 < np.mean(want) < 0.9
    path = tmp_path / "rays.f32"
    rays.tofile(path)
    for prog in programs:
        assert [int(x) for x in run(prog, "rays", path).split()] == [int(w) for w in want]

    unit = ((0, 0, 0), (1, 1, 1))
    flat = ((0, 0, 0), (1, 0, 1))
    nan = ((np.nan,) * 3, (np.nan,) * 3)
    scenes = {
        "ordered": [quad_node([unit, flat, unit, unit], 0xf)],
        "empty": [],
        "inverted box": [quad_node([unit] * 4, 0xf), quad_node([unit, ((0, 2, 0), (1, 1, 1)), unit, unit], 0xf)],
        "inverted box in an invalid slot": [quad_node([unit, ((1, 1, 1), (-1, -1, -1)), unit, unit], 0xd)],
        "infinite plane": [quad_node([unit, unit, ((0, 0, -np.inf), (1, 1, 1)), unit], 0xf)],
        "infinite hi": [quad_node([unit, unit, unit, ((0, 0, 0), (1, np.inf, 1))], 0xf)],
        "NaN in a valid slot": [quad_node([unit, unit, unit, ((0, 0, 0), (1, np.nan, 1))], 0xf)],
        "NaN in an invalid slot": [quad_node([unit, nan, unit, nan], 0x5)],
        "NaN in slot 3, invalid, after an ordered node": [quad_node([unit] * 4, 0xf), quad_node([unit, unit, unit, nan], 0x7)],
    }
    expect = {"ordered": True, "empty": True, "inverted box": False, "inverted box in an invalid slot": True, "infinite plane": False,
              "infinite hi": False, "NaN in a valid slot": False, "NaN in an invalid slot": True,
              "NaN in slot 3, invalid, after an ordered node": True}
    for name, nodes in scenes.items():
        quad = np.concatenate(nodes).astype(np.float32) if nodes else np.zeros(0, np.float32)
        assert scene_foldable(quad) == expect[name], name
        path = tmp_path / "scene.f32"
        quad.tofile(path)
        for prog in programs:
            assert int(run(prog, "scene", path)) == int(expect[name]), name
