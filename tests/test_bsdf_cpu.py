"""The scattering layer without a GPU.

(a) pbr_hip_bsdf_host — the device's BSDF functions (pbr_device.h, under each production lobe mask)
    compiled for the CPU — against the oracle's BSDF::f / Pdf / Sample_f, bit for bit: both sides are
    IEEE float32 without contraction and take their transcendentals from this machine's libm through
    (float)f((double)x), so there is no tolerance.  Within the host output, the fused bsdf_f_pdf (given
    Lambda(wo) or not) equals bsdf_f / bsdf_pdf and the split bsdf_sample_dir + bsdf_sample_sum equals
    bsdf_sample.
(b) the oracle against tests/bsdf_expected.py, a float64 statement written from the formulas, under
    rel_bound(material) — four times the largest relative difference measured over this query set for
    that material (MEASURED_MAX).  A query is left out only by bsdf_expected.ill_conditioned, which looks at the
    inputs, and the rule may leave out at most 5% of a material's queries.
(c) the Henyey-Greenstein pair the same way.
"""
import ctypes as C

import numpy as np
import pytest

import bsdf_expected as bx
import bsdf_queries as bq
import oracle_lib
from pysicalbasedraytracer_amd import capi, scenes

# largest relative difference oracle (float32) vs bsdf_expected (float64) over the query set, measured
# on the CPU (every material, both allowMultipleLobes values); the bound is four times it, since a
# maximum over a finite set moves with the seed
MEASURED_MAX = {
    "matte": 2.70e-06, "matte_sigma20": 2.70e-06, "matte_black": 0.0, "mirror": 1.92e-06, "glass_smooth": 1.41e-04,
    "glass_rough": 9.03e-05, "glass_aniso": 9.02e-05, "glass_remap": 9.04e-05, "glass_kr_black": 9.03e-05,
    "glass_kt_black": 4.17e-05, "glass_smooth_kr_black": 6.27e-04, "metal": 1.58e-05, "metal_aniso": 5.85e-05,
    # alphas at the 0.001 clamp: D varies over angles of 1e-3, where a float32 direction carries 1e-4 of that
    "metal_tiny": 3.89e-01, "metal_tiny_remap": 1.81e-04, "plastic": 1.00e-05, "plastic_ks_black": 2.70e-06, "none": 0.0,
}
# per |g|; at 0.999 the denominator 1 + g^2 + 2 g cos cancels to 1e-6 of its terms in float32
MEASURED_MAX_HG = {0.0: 1.06e-07, 1e-4: 1.80e-07, 0.3: 5.09e-07, 0.9: 1.41e-05, 0.999: 3.12e-01}

L_LAMBERT, L_OREN, L_SPEC_R, L_SPEC_T, L_FRESNEL_SPEC, L_MF_R, L_MF_T = range(7)
SIMPLE = (1 << L_LAMBERT) | (1 << L_OREN) | (1 << L_SPEC_R) | (1 << L_SPEC_T) | (1 << L_FRESNEL_SPEC)
VARIANT_MASKS = {
    capi.BSDF_VARIANT_ALL: 0x7f, capi.BSDF_VARIANT_SIMPLE: SIMPLE,
    capi.BSDF_VARIANT_MATTE_MIRROR: (1 << L_LAMBERT) | (1 << L_SPEC_R),
    capi.BSDF_VARIANT_MICRO: (1 << L_LAMBERT) | (1 << L_MF_R) | (1 << L_MF_T),
    capi.BSDF_VARIANT_PASS_L: 1 << L_LAMBERT, capi.BSDF_VARIANT_PASS_R: 1 << L_MF_R,
    capi.BSDF_VARIANT_PASS_LR: (1 << L_LAMBERT) | (1 << L_MF_R), capi.BSDF_VARIANT_PASS_RT: (1 << L_MF_R) | (1 << L_MF_T),
    capi.BSDF_VARIANT_PASS_LRT: (1 << L_LAMBERT) | (1 << L_MF_R) | (1 << L_MF_T), capi.BSDF_VARIANT_MIRROR: 1 << L_SPEC_R,
    capi.BSDF_VARIANT_TEXTURED: 0xff, capi.BSDF_VARIANT_ALL_LDS: 0x7f, capi.BSDF_VARIANT_ALL_GLOBAL: 0x7f,
}
KIND_BITS = {"lambert": L_LAMBERT, "oren": L_OREN, "spec_r": L_SPEC_R, "spec_t": L_SPEC_T, "fresnel_spec": L_FRESNEL_SPEC,
             "mf_r": L_MF_R, "mf_t": L_MF_T}
FIELDS = ("no_bsdf", "f", "pdf", "f_lam", "pdf_lam", "f_nolam", "pdf_nolam", "s_wi", "s_f", "s_pdf", "s_type", "d_wi", "d_f",
          "d_pdf", "d_type")


def rel_bound(name):
    return 4 * MEASURED_MAX.get(name, 0.0)


def material_mask(name):
    """The lobe kinds of a material over both allowMultipleLobes values (what a variant must cover)."""
    m = 0
    for multi in (0, 1):
        for l in bx.lobes(name, multi) or ():
            m |= 1 << KIND_BITS[l["kind"]]
    return m


def admissible(name):
    return [v for v, mask in VARIANT_MASKS.items() if material_mask(name) & ~mask == 0]


def bits_differ(a, b, field, wi_live=None):
    """Rows where field differs as uint32 words: two NaNs are equal, -0 and +0 are not.  wi_live: for a
    sampled direction, the rows where it is defined (the sample's pdf is not 0)."""
    x = np.ascontiguousarray(a[field]).reshape(len(a), -1)
    y = np.ascontiguousarray(b[field]).reshape(len(b), -1)
    ne = x.view(np.uint32) != y.view(np.uint32)
    if x.dtype.kind == "f":
        ne &= ~(np.isnan(x) & np.isnan(y))
    ne = ne.any(1)
    return ne & wi_live if wi_live is not None else ne


def assert_records_equal(a, b, what, fields=FIELDS):
    for fld in fields:
        live = None
        if fld in ("s_wi", "d_wi"):
            live = a["s_pdf" if fld == "s_wi" else "d_pdf"] != 0
        ne = bits_differ(a, b, fld, live)
        assert not ne.any(), f"{what}: {fld} differs in {int(ne.sum())} of {len(a)} queries, first {int(np.argmax(ne))}: " \
                             f"{a[fld][np.argmax(ne)]} vs {b[fld][np.argmax(ne)]}"


def assert_self_consistent(r, what):
    """Within one output: the fused forms equal bsdf_f / bsdf_pdf, the split sample equals bsdf_sample."""
    for fused_f, fused_pdf in (("f_lam", "pdf_lam"), ("f_nolam", "pdf_nolam")):
        for x, y in (("f", fused_f), ("pdf", fused_pdf)):
            a = np.ascontiguousarray(r[x]).reshape(len(r), -1)
            b = np.ascontiguousarray(r[y]).reshape(len(r), -1)
            ne = ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any(1)
            assert not ne.any(), f"{what}: {y} != {x} in {int(ne.sum())} queries, first {int(np.argmax(ne))}"
    for x, y in (("s_wi", "d_wi"), ("s_f", "d_f"), ("s_pdf", "d_pdf"), ("s_type", "d_type")):
        a = np.ascontiguousarray(r[x]).reshape(len(r), -1)
        b = np.ascontiguousarray(r[y]).reshape(len(r), -1)
        ne = a.view(np.uint32) != b.view(np.uint32)
        if a.dtype.kind == "f":
            ne &= ~(np.isnan(a) & np.isnan(b))
        ne = ne.any(1)
        if x == "s_wi":
            ne &= r["s_pdf"] != 0
        assert not ne.any(), f"{what}: {y} != {x} in {int(ne.sum())} queries, first {int(np.argmax(ne))}"
    # bsdf_sample_dir returns false exactly where Sample_f returns black before the sum
    dead = r["d_ok"] == 0
    assert not (r["s_f"][dead & (r["no_bsdf"] == 0)] != 0).any(), what


_cache = {}


def case(name, multi):
    """(scene, queries, oracle records) of one material, computed once."""
    key = (name, multi)
    if key not in _cache:
        s = scenes.Scene()
        m = bq.add_material(s, name)
        q = bq.build(m, multi)
        q.setflags(write=False)
        o = oracle_lib.bsdf(s, q)
        o.setflags(write=False)
        _cache[key] = (s, q, o)
    return _cache[key]


CASES = [(name, multi) for name in bq.MATERIALS for multi in (0, 1)]


# ------------------------------------------------------------------ (a) host twin vs oracle
@pytest.mark.parametrize("name,multi", CASES)
def test_host_twin_equals_oracle_bit_for_bit(name, multi):
    s, q, o = case(name, multi)
    variants = admissible(name)
    assert capi.BSDF_VARIANT_ALL in variants
    for v in variants:
        h = capi.bsdf_host(s.materials[0], v, q)
        assert_records_equal(h, o, f"{name} multi={multi} variant={v}")
        assert_self_consistent(h, f"{name} multi={multi} variant={v}")


def test_host_twin_single_query():
    s, q, o = case("plastic", 1)
    h = capi.bsdf_host(s.materials[0], capi.BSDF_VARIANT_MICRO, q[:1])
    assert_records_equal(h, o[:1], "n = 1")


def test_every_variant_is_admissible_for_some_material():
    seen = set()
    for name in bq.MATERIALS:
        seen.update(admissible(name))
    assert seen == set(VARIANT_MASKS)


def test_sentinels_survive_the_tangent_plane_early_out():
    """BSDF::Sample_f leaves *pdf and the sampled type untouched when wo.z == 0 (Reflection.cpp:121)."""
    s, q, o = case("plastic", 1)
    fr = bx.Frame(q)
    in_plane = (fr.to_local(q["wo"].astype(np.float64))[:, 2] == 0) & (q["type"] == capi.BSDF_ALL)
    assert in_plane.sum() >= 4
    h = capi.bsdf_host(s.materials[0], capi.BSDF_VARIANT_ALL, q)
    for r in (h, o):
        assert (r["s_pdf"][in_plane] == -1).all() and (r["s_type"][in_plane] == -1).all()
        assert (r["s_f"][in_plane] == 0).all()
    assert (h["d_ok"][in_plane] == 0).all()


def test_refusals():
    lib = capi.load_library()
    q = case("glass_rough", 1)[1][:3].copy()
    out = np.zeros(3, dtype=capi.bsdf_record_dtype())
    qp, op = q.ctypes.data, out.ctypes.data
    glass = bq.material_desc("glass_rough")
    # a mask that does not cover the material
    for v in (capi.BSDF_VARIANT_SIMPLE, capi.BSDF_VARIANT_MATTE_MIRROR, capi.BSDF_VARIANT_PASS_L, capi.BSDF_VARIANT_PASS_R,
              capi.BSDF_VARIANT_PASS_LR, capi.BSDF_VARIANT_MIRROR):
        assert lib.pbr_hip_bsdf_host(C.byref(glass), v, 3, qp, op) == capi.PBR_E_INVALID, v
    assert lib.pbr_hip_bsdf_host(C.byref(bq.material_desc("matte_sigma20")), capi.BSDF_VARIANT_MATTE_MIRROR, 3, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(bq.material_desc("glass_smooth")), capi.BSDF_VARIANT_MATTE_MIRROR, 3, qp, op) == capi.PBR_E_INVALID
    # an unknown variant, an unknown material type, an image-textured material
    for v in (-1, 13, 1000):
        assert lib.pbr_hip_bsdf_host(C.byref(glass), v, 3, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(capi.MaterialDesc(type=17)), capi.BSDF_VARIANT_ALL, 3, qp, op) == capi.PBR_E_INVALID
    tex = bq.material_desc("matte")
    tex.tex[capi.TEX_KD] = 1
    assert lib.pbr_hip_bsdf_host(C.byref(tex), capi.BSDF_VARIANT_TEXTURED, 3, qp, op) == capi.PBR_E_INVALID
    # NULL arguments, negative n; n = 0 needs no arrays
    assert lib.pbr_hip_bsdf_host(None, capi.BSDF_VARIANT_ALL, 3, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(glass), capi.BSDF_VARIANT_ALL, 3, None, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(glass), capi.BSDF_VARIANT_ALL, 3, qp, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(glass), capi.BSDF_VARIANT_ALL, -1, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf_host(C.byref(glass), capi.BSDF_VARIANT_ALL, 0, None, None) == capi.PBR_OK
    assert lib.pbr_hip_phase_hg_host(1, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_phase_hg_host(-1, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_phase_hg_host(0, None, None) == capi.PBR_OK
    # a query whose material is not the one given has no BSDF
    q["material"] = (1, -1, 0)
    h = capi.bsdf_host(glass, capi.BSDF_VARIANT_ALL, q)
    assert list(h["no_bsdf"]) == [1, 1, 0]


# ------------------------------------------------------------------ (b) oracle vs the float64 statement
def rel_diff(got, want):
    """|got - want| / |want| per row (the largest over a row's channels); want == 0 demands got == 0,
    reported as inf."""
    got = np.asarray(got, np.float64).reshape(len(got), -1)
    want = np.asarray(want, np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(want == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - want) / np.abs(want))
    return np.where(np.isnan(r), np.inf, r).max(1)


def float64_differences(name, multi):
    """The relative differences oracle vs float64 of one material: a dict of per-row arrays (rows the
    conditioning rule leaves out hold 0) and the share of rows it left out."""
    s, q, o = case(name, multi)
    ls = bx.lobes(name, multi)
    if ls is None:
        assert (o["no_bsdf"] == 1).all()
        return {}, 0.0
    assert (o["no_bsdf"] == 0).all()
    out = {}
    skip = bx.ill_conditioned(ls, q)
    out["f"] = np.where(skip, 0.0, rel_diff(o["f"], bx.bsdf_f(ls, q)))
    out["pdf"] = np.where(skip, 0.0, rel_diff(o["pdf"], bx.bsdf_pdf(ls, q)))
    # the sample: the float64 pdf and f at the returned direction; a specular lobe's direction and weight
    fr = bx.Frame(q)
    wo = fr.to_local(q["wo"].astype(np.float64))
    live = (o["s_pdf"] > 0) & (wo[:, 2] != 0)
    swi = o["s_wi"].astype(np.float64)
    skip_s = bx.ill_conditioned(ls, q, swi) | ~live
    spec = [l for l in ls if l["type"] & bx.SPEC]
    if not spec:
        out["s_pdf"] = np.where(skip_s, 0.0, rel_diff(o["s_pdf"], bx.bsdf_pdf(ls, q, swi)))
        out["s_f"] = np.where(skip_s, 0.0, rel_diff(o["s_f"], bx.bsdf_f(ls, q, swi)))
    else:
        assert len(spec) == len(ls)   # the materials' specular lobes come alone
        matching = [bx._matches(l, q["type"]) for l in ls]
        m = sum(x.astype(int) for x in matching)
        comp = np.minimum(np.floor(q["u0"].astype(np.float64) * m), m - 1)
        chosen = np.zeros(len(q), int)
        if len(ls) == 2:   # the comp-th matching lobe
            chosen = np.where(matching[0] & (comp == 0), 0, 1)
        wi64, f64, pdf64, type64 = (np.zeros((len(q), 3)), np.zeros((len(q), 3)), np.zeros(len(q)), np.zeros(len(q), int))
        for k, l in enumerate(ls):
            rb = (o["s_type"] & bx.REFL) != 0   # FresnelSpecular: the branch taken, checked against u0 below
            w, f, p, t = bx.specular_sample(l, wo, rb)
            pick = (chosen == k) & matching[k]
            wi64[pick], f64[pick], pdf64[pick], type64[pick] = w[pick], f[pick], (p / np.maximum(m, 1))[pick], t[pick]
            if l["kind"] == "fresnel_spec":
                F = bx.fr_dielectric(wo[:, 2], l["etaA"], l["etaB"])
                ur = np.minimum(q["u0"].astype(np.float64) * m - comp, float(bq.ONE_MINUS_EPS))
                ok = np.where(rb, ur < F * (1 + rel_bound(name)), ur >= F * (1 - rel_bound(name)))
                assert ok[pick & live].all(), f"{name}: FresnelSpecular took the wrong branch"
        assert (o["s_type"][live] == type64[live]).all(), name
        out["s_pdf"] = np.where(skip_s, 0.0, rel_diff(o["s_pdf"], pdf64))
        out["s_f"] = np.where(skip_s, 0.0, rel_diff(o["s_f"], f64))
        # the direction: absolute, in units of a unit vector
        out["s_wi"] = np.where(skip_s, 0.0, np.abs(fr.to_local(swi) - wi64).max(1))
        # where float64 says a sample exists (away from the rule), the oracle has one
        exists = (pdf64 > 0) & ~bx.ill_conditioned(ls, q, fr.to_world(wi64)) & (m > 0)
        assert (o["s_pdf"][exists] > 0).all(), name
    share = max(float(skip.mean()), float((skip_s & live).sum()) / max(1, int(live.sum())))
    return out, share


@pytest.mark.parametrize("name,multi", CASES)
def test_oracle_matches_float64_statement(name, multi):
    diffs, share = float64_differences(name, multi)
    print(f"{name} multi={multi}: left out {share:.4f}; " + ", ".join(f"{k} {v.max():.3g}" for k, v in diffs.items()))
    assert share <= 0.05, f"the conditioning rule leaves out {share:.3f} of the queries"
    for k, v in diffs.items():
        assert v.max() <= rel_bound(name), f"{name} multi={multi}: {k} differs by {v.max():.3g} at query {int(np.argmax(v))}"


def test_float64_pdfs_integrate_to_at_most_one():
    """The statement itself: each non-specular lobe's pdf over the sphere of wi is <= 1 for three wo,
    and 1 where sampling cannot fail (the cosine lobes; a rough reflector seen near the normal)."""
    n_t, n_p = 1500, 720
    c = -1 + (np.arange(n_t) + 0.5) * (2.0 / n_t)            # midpoint rule in (cos theta, phi)
    p = (np.arange(n_p) + 0.5) * (2 * np.pi / n_p)
    cc, pp = np.meshgrid(c, p, indexing="ij")
    s = np.sqrt(1 - cc ** 2)
    wi = np.stack([s * np.cos(pp), s * np.sin(pp), cc], -1).reshape(-1, 3)
    dw = (2.0 / n_t) * (2 * np.pi / n_p)
    alpha = 0.3
    lobes = {
        "lambert": dict(kind="lambert", type=5, R=np.ones(3)),
        "oren": dict(kind="oren", type=5, R=np.ones(3), A=0.9, B=0.2),
        "mf_r": dict(kind="mf_r", type=9, R=np.ones(3), ax=alpha, ay=alpha, fresnel=None),
        "mf_t": dict(kind="mf_t", type=10, T=np.ones(3), ax=alpha, ay=alpha, etaA=1.0, etaB=1.5),
    }
    for wo in ((0.0, 0.0, 1.0), (0.48, -0.36, 0.8), (-0.6, 0.64, -0.48)):
        wo_a = np.broadcast_to(np.asarray(wo), wi.shape)
        for kind, l in lobes.items():
            pdf = bx.lobe_pdf(l, wo_a, wi)
            if kind == "mf_t":
                # the reference's transmission pdf takes |wo.wh|: it also covers half vectors facing away
                # from wo, which the visible-normal sampling never produces; those are left out here
                pdf = np.where(bx._dot(wo_a, bx._mf_t_half(l, wo_a, wi)[1]) * wo[2] > 0, pdf, 0.0)
            total = float(np.nansum(pdf) * dw)
            print(f"integral of the {kind} pdf for wo = {wo}: {total:.5f}")
            # (from inside, beyond the critical angle, most facets reflect totally: the transmission is small)
            assert 0.1 < total <= 1 + 2e-3, (kind, wo, total)
            if kind in ("lambert", "oren"):   # every sample is a direction of the hemisphere
                assert abs(total - 1) <= 2e-3, (kind, wo, total)
            elif kind == "mf_r" and wo[2] == 1.0:
                # seen along the normal every facet is visible, and its mirror direction stays above the
                # surface while the facet tilts less than 45 degrees: the mass of D cos there, 1 / (1 + alpha^2)
                assert abs(total - 1 / (1 + alpha ** 2)) <= 2e-3, (kind, wo, total)


# ------------------------------------------------------------------ (c) Henyey-Greenstein
def test_phase_hg_host_twin_equals_oracle_bit_for_bit():
    q = bq.build_phase()
    h, o = capi.phase_hg_host(q), oracle_lib.phase_hg(q)
    ne = (h.view(np.uint32) != o.view(np.uint32)) & ~(np.isnan(h) & np.isnan(o))
    assert not ne.any(), f"{int(ne.any(1).sum())} of {len(q)} differ, first {int(np.argmax(ne.any(1)))}"
    assert np.isfinite(h).all()
    one = capi.phase_hg_host(q[:1])
    assert (one.view(np.uint32) == o[:1].view(np.uint32)).all()


def phase_hg_differences():
    """Per |g|: the largest differences oracle vs float64 — relative for p(wo, wi) and the sampled
    direction's value, absolute for its cosine to wo and its length."""
    q = bq.build_phase().astype(np.float64)
    o = oracle_lib.phase_hg(q.astype(np.float32)).astype(np.float64)
    g, wo, wi = q[:, 0], q[:, 1:4], q[:, 4:7]
    swi = o[:, 1:4]
    u0 = q[:, 7]
    # Sample_p: a unit vector whose cosine to wo is the inverse of the HG cdf at u0 (isotropic below
    # |g| = 1e-3), and the phase value of that cosine
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_hg = -(1 + g * g - ((1 - g * g) / (1 + g - 2 * g * u0)) ** 2) / (2 * g)
    cos64 = np.where(np.abs(g) < 1e-3, 1 - 2 * u0, cos_hg)
    d = np.stack([rel_diff(o[:, 0], bx.phase_hg(np.sum(wo * wi, 1), g)), rel_diff(o[:, 4], bx.phase_hg(cos64, g)),
                  np.abs(np.sum(wo * swi, 1) - cos64), np.abs(np.linalg.norm(swi, axis=1) - 1)], 1)
    return {float(a): d[np.abs(g) == a].max(0) for a in np.unique(np.abs(g))}


def test_phase_hg_oracle_matches_float64():
    for a, d in phase_hg_differences().items():
        print(f"HG |g| = {a:g}: p {d[0]:.3g}, sampled value {d[1]:.3g}, cosine {d[2]:.3g}, length {d[3]:.3g}")
        bound = 4 * MEASURED_MAX_HG[round(a, 4)]
        assert d.max() <= bound, (a, d, bound)
