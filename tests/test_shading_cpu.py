"""Per-vertex shading normals without a GPU: pbr_hip_shading_host (the hit path's frame function of
csrc/pbr_shading_frame.h compiled for the host) against the float32 numpy restatement of the
reference's lines (shading_expected.py) on the bits, and the Python layer that carries normals."""
import ctypes as C
import struct

import numpy as np
import pytest

import shading_expected as SE
from pysicalbasedraytracer_amd import capi, scenes

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def query(p, n, b, uv=None, reverse=0, swaps=0):
    q = np.zeros(1, dtype=capi.shading_query_dtype())
    q["p"], q["n"], q["b"] = np.asarray(p, dtype=f32), np.asarray(n, dtype=f32), np.asarray(b, dtype=f32)
    if uv is not None:
        q["uv"], q["has_uv"] = np.asarray(uv, dtype=f32), 1
    q["reverse_orientation"], q["swaps_handedness"] = reverse, swaps
    return q


TRI = [(0, 0, 0), (2, 0, 0), (0, 1, 0)]          # geometric normal Cross(p0 - p2, p1 - p2) = (0, 0, 2) → +z
B = (0.25, 0.25, 0.5)


def crafted_queries():
    """The branches of the frame, each under the four reverse × swaps combinations."""
    up, down = [(0, 0, 1)] * 3, [(0, 0, -1)] * 3
    cases = {
        "plain": dict(p=TRI, n=[(0.1, 0, 1), (0, 0.2, 1), (-0.1, -0.1, 1)], b=B),
        # b0 n0 + b1 n1 + b2 n2 = 0 exactly: ns falls back to n
        "normals_cancel": dict(p=TRI, n=[(1, 0, 0), (-1, 0, 0), (0, 0, 0)], b=B),
        "normals_zero": dict(p=TRI, n=[(0, 0, 0)] * 3, b=B),
        # one UV for all vertices: dpdu = (0, 0, 0), ss = NaN, ts = NaN → CoordinateSystem(ns)
        "degenerate_uv": dict(p=TRI, n=[(0.1, 0, 1), (0, 0.2, 1), (-0.1, -0.1, 1)], b=B, uv=[(0.5, 0.5)] * 3),
        "degenerate_uv_x_major": dict(p=TRI, n=[(1, 0.1, 0.2)] * 3, b=B, uv=[(0.5, 0.5)] * 3),
        # default UVs give dpdu = p1 - p0 = (2, 0, 0); ns = (1, 0, 0) is parallel to it: ts = 0 → CoordinateSystem(ns)
        "ns_parallel_to_dpdu": dict(p=TRI, n=[(1, 0, 0)] * 3, b=B),
        "ns_antiparallel_to_dpdu": dict(p=TRI, n=[(-3, 0, 0)] * 3, b=B),
        # normals on the far side of the geometric normal: n flips to follow ns
        "far_side": dict(p=TRI, n=down, b=B),
        "far_side_tilted": dict(p=TRI, n=[(0.3, 0.1, -1), (0, 0.2, -1), (-0.1, 0.4, -1)], b=B),
        "near_side": dict(p=TRI, n=up, b=B),
        # unnormalised normals (a non-uniform scale leaves them so), a vertex hit and an edge hit
        "long_normals": dict(p=TRI, n=[(0, 0, 7.5), (0.5, 0, 3), (0, 2, 0.25)], b=B),
        "vertex_hit": dict(p=TRI, n=[(0.1, 0, 1), (0, 0.2, 1), (-0.1, -0.1, 1)], b=(0, 1, 0)),
        "edge_hit": dict(p=TRI, n=[(0.1, 0, 1), (0, 0.2, 1), (-0.1, -0.1, 1)], b=(0.5, 0, 0.5)),
    }
    names, qs = [], []
    for name, kw in cases.items():
        for reverse in (0, 1):
            for swaps in (0, 1):
                names.append(f"{name}/reverse={reverse}/swaps={swaps}")
                qs.append(query(reverse=reverse, swaps=swaps, **kw))
    return names, np.concatenate(qs)


def random_queries(n, seed=7):
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=capi.shading_query_dtype())
    q["p"] = rng.uniform(-3, 3, (n, 3, 3)).astype(f32)
    ng = np.cross(q["p"][:, 0] - q["p"][:, 2], q["p"][:, 1] - q["p"][:, 2])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    # a third each: normals about the geometric one, about its negative, and anywhere; lengths 0.2 … 5
    kind = rng.integers(0, 3, n)
    base = np.where(kind[:, None] == 0, ng, np.where(kind[:, None] == 1, -ng, 0.0))
    nrm = base[:, None, :] + rng.normal(0, 0.4, (n, 3, 3)) * np.where(kind == 2, 2.5, 1.0)[:, None, None]
    q["n"] = (nrm * rng.uniform(0.2, 5.0, (n, 3, 1))).astype(f32)
    b = rng.dirichlet((1, 1, 1), n)
    q["b"] = b.astype(f32)
    q["uv"] = rng.uniform(-2, 2, (n, 3, 2)).astype(f32)
    q["has_uv"] = rng.integers(0, 2, n)
    q["reverse_orientation"] = rng.integers(0, 2, n)
    q["swaps_handedness"] = rng.integers(0, 2, n)
    return q


def test_the_host_frame_equals_the_restatement_bit_for_bit():
    names, crafted = crafted_queries()
    rand = random_queries(2000 - crafted.shape[0])
    q = np.concatenate([crafted, rand])
    names += [f"random {i}" for i in range(rand.shape[0])]
    got = capi.shading_host(q)
    want = SE.expected_of_queries(q)
    assert got.shape == want.shape == (2000, 3, 3)
    assert np.isfinite(got).all() and np.isfinite(want).all(), "every case has a finite frame"
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(2000, -1).any(axis=1))
    assert bad.size == 0, f"{bad.size} queries differ, first: {names[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    # the reverse × swaps combinations are all drawn, with and without UVs
    combos = {(int(r), int(s), int(u)) for r, s, u in zip(rand["reverse_orientation"], rand["swaps_handedness"], rand["has_uv"])}
    assert len(combos) == 8


def test_the_crafted_cases_take_the_branches_they_name():
    """The restatement's own intermediate values on the crafted cases (so a case cannot silently stop covering
    its branch), and what the reference's lines imply for the result."""
    names, q = crafted_queries()
    got = capi.shading_host(q)
    uv = np.where(q["has_uv"][:, None, None] != 0, q["uv"], SE.DEFAULT_UV[None]).astype(f32)
    rev, swp = q["reverse_orientation"] != 0, q["swaps_handedness"] != 0
    ng, dpdu = SE.frame_inputs(q["p"], uv, rev ^ swp)
    for i, name in enumerate(names):
        n, ns, ss = got[i]
        ns_sum = SE.lerp3(q["b"][i:i + 1], q["n"][i:i + 1])[0]
        if name.startswith(("normals_cancel", "normals_zero")):
            assert not ns_sum.any()
            assert np.array_equal(np.abs(ns), (0, 0, 1)), name   # the frame's normal is ±n
        if name.startswith("degenerate_uv"):
            assert not dpdu[i].any() and np.isnan(SE.normalize(dpdu[i:i + 1])).all()
        if "parallel_to_dpdu" in name:
            unit = SE.normalize(ns_sum[None])
            assert not SE.cross(SE.normalize(dpdu[i:i + 1]), unit).any()
        if name.startswith("far_side"):   # (under the reverse ^ swaps flip, "near_side" is the far one)
            assert np.dot(ng[i], ns_sum) * (-1 if rev[i] ^ swp[i] else 1) < 0
        # SetShadingGeometry, orientationIsAuthoritative: n is ±(geometric n), on shading.n's side
        assert np.array_equal(np.abs(n), np.abs(ng[i])), name
        assert np.dot(n.astype(np.float64), ns.astype(np.float64)) >= 0, name
        # the frame is orthonormal: ss is unit and perpendicular to shading.n
        assert abs(float(np.linalg.norm(ss.astype(np.float64))) - 1) < 1e-6, name
        assert abs(float(np.dot(ss.astype(np.float64), ns.astype(np.float64)))) < 1e-6, name
    # reverseOrientation alone flips ts and with it shading.n: same query, reverse toggled, swaps toggled too so
    # that the geometric flip (reverse ^ swaps) stays
    by = dict(zip(names, got))
    a, b = by["plain/reverse=0/swaps=0"], by["plain/reverse=1/swaps=1"]
    assert np.array_equal(a[1], -b[1]) and np.array_equal(a[2], b[2])   # (as values: a zero component keeps its sign)
    assert np.array_equal(a[0], -b[0]), "n follows shading.n"


def test_the_entry_point_checks_its_arguments():
    lib = capi.load_library()
    out = np.zeros(9, dtype=f32)
    q = query(TRI, [(0, 0, 1)] * 3, B)
    assert lib.pbr_hip_shading_host(0, None, None) == capi.PBR_OK
    assert lib.pbr_hip_shading_host(-1, q.ctypes.data, out.ctypes.data) == capi.PBR_E_INVALID
    assert lib.pbr_hip_shading_host(1, None, out.ctypes.data) == capi.PBR_E_INVALID
    assert lib.pbr_hip_shading_host(1, q.ctypes.data, None) == capi.PBR_E_INVALID
    assert capi.shading_query_dtype().itemsize == 128


def test_scene_mesh_carries_normals():
    s = scenes.Scene()
    P, I, N = scenes.dragon_standin(n=4, normals=True)
    m = s.matte((0.5, 0.5, 0.5))
    with_n = s.mesh(P, I, m, normals=N)
    flat = s.mesh(P, I, m)
    sd = s.shapes[with_n]
    assert sd.N and not s.shapes[flat].N
    back = np.ctypeslib.as_array(sd.N, shape=(sd.n_vertices * 3,)).reshape(-1, 3)
    assert np.array_equal(bits(back), bits(N))
    # any array-like, converted to float32
    sd2 = s.shapes[s.mesh(P, I, m, normals=N.astype(np.float64).tolist())]
    assert np.array_equal(np.ctypeslib.as_array(sd2.N, shape=(sd2.n_vertices * 3,)), N.reshape(-1))
    with pytest.raises(ValueError, match="per vertex"):
        s.mesh(P, I, m, normals=N[:-1])
    light = s.area_light_mesh(P[:3], np.array([[0, 1, 2]], np.int32), (1, 1, 1), m, normals=N[:3], reverse=True)
    assert s.shapes[light].N and s.shapes[light].reverse_orientation == 1


def test_dragon_standin_normals_are_the_radius_function_gradient():
    P0, I0 = scenes.dragon_standin(n=12)
    P, I, N = scenes.dragon_standin(n=12, normals=True)
    assert np.array_equal(P, P0) and np.array_equal(I, I0), "the mesh itself is unchanged"
    assert N.dtype == np.float32 and N.shape == P.shape
    assert np.abs(np.linalg.norm(N.astype(np.float64), axis=1) - 1).max() < 1e-6
    # central differences of the implicit function |x| − r(θ, φ) at the vertices off the pole rows
    def F(x):
        rho = np.linalg.norm(x, axis=1)
        t = np.arccos(np.clip(x[:, 1] / rho, -1, 1))
        p = np.arctan2(x[:, 2], x[:, 0])
        return rho - (1.0 + 0.08 * np.sin(7 * t) * np.cos(9 * p) + 0.03 * np.sin(31 * t + 17 * p))
    X = P.astype(np.float64)[12:-12]
    h = 1e-6
    G = np.stack([(F(X + h * e) - F(X - h * e)) / (2 * h) for e in np.eye(3)], axis=1)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    assert np.abs(G - N[12:-12]).max() < 1e-4   # (float32 vertices: the angles are known to ~1e-7, r' is below 1.5)


PLY_V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], dtype=f32)
PLY_N = np.array([(0, 0, 1), (0.125, 0, 0.75), (0, -0.5, 1), (0.25, 0.25, -1)], dtype=f32)
PLY_F = [(0, 1, 2), (1, 3, 2)]


def write_ply(path, binary, with_normals):
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    head = ["ply", "format " + ("binary_little_endian 1.0" if binary else "ascii 1.0"), f"element vertex {len(PLY_V)}"]
    head += [f"property float {p}" for p in props]
    head += [f"element face {len(PLY_F)}", "property list uchar int vertex_indices", "end_header"]
    rows = np.concatenate([PLY_V, PLY_N], axis=1) if with_normals else PLY_V
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            fh.write(rows.astype("<f4").tobytes())
            for f in PLY_F:
                fh.write(struct.pack("<B3i", 3, *f))
        else:
            for r in rows:
                fh.write((" ".join(repr(float(v)) for v in r) + "\n").encode("ascii"))
            for f in PLY_F:
                fh.write(("3 " + " ".join(str(i) for i in f) + "\n").encode("ascii"))


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
def test_load_ply_returns_the_files_normals(tmp_path, binary):
    path = str(tmp_path / "n.ply")
    write_ply(path, binary, True)
    V, F, N = scenes.load_ply(path, normals=True)
    assert np.array_equal(bits(V), bits(PLY_V)) and np.array_equal(F, np.asarray(PLY_F, np.int32))
    assert N.dtype == np.float32 and np.array_equal(bits(N), bits(PLY_N))
    assert len(scenes.load_ply(path)) == 2, "the default call returns (V, F)"
    plain = str(tmp_path / "plain.ply")
    write_ply(plain, binary, False)
    V2, F2, N2 = scenes.load_ply(plain, normals=True)
    assert N2 is None and np.array_equal(V2, PLY_V)
