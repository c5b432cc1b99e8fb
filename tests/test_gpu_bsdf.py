"""The scattering layer on the device: pbr_hip_bsdf and pbr_hip_phase_hg against the oracle on the
queries of tests/bsdf_queries.py, under every lobe mask and template source the shading kernels are
compiled with (one uploaded scene per lobe-kind set, so each variant is admissible somewhere).

Compared as uint32 words (two NaNs equal, -0 and +0 not).  A field whose path reaches no
transcendental must be bit-identical without exception.  A sampled direction comes through double
sin / cos where the chosen lobe is a cosine lobe or a microfacet lobe seen within cos > .9999 of the
stretched normal, Sample_p always does, and an image-textured roughness goes through a double log:
there the device's libm may round differently from glibc's at a float rounding boundary, so at most
1 in 1000 of those queries may differ, each by at most one float ulp.  Expected and observed: 0
(DESIGN.md §4.6).  The device's own fused, unfused and split outputs, its LDS and global template
reads and its variants must equal each other with no allowance.
"""
import ctypes as C

import numpy as np
import pytest

import bsdf_expected as bx
import bsdf_queries as bq
import oracle_lib
import ref_scenes as RS
from pysicalbasedraytracer_amd import HipRenderer, capi, scenes
from test_bsdf_cpu import FIELDS, VARIANT_MASKS, assert_records_equal, assert_self_consistent, bits_differ, material_mask

pytestmark = pytest.mark.gpu

SAMPLE_FIELDS = ("s_wi", "s_f", "s_pdf", "s_type", "d_wi", "d_f", "d_pdf", "d_type")
SCENES = {
    "matte_mirror": ["matte", "mirror", "matte_black", "none"],
    "simple": ["matte_sigma20", "glass_smooth", "glass_smooth_kr_black", "mirror", "matte"],
    "micro": ["matte", "plastic", "metal", "metal_aniso", "glass_rough", "glass_aniso", "glass_remap", "glass_kr_black",
              "glass_kt_black", "metal_tiny", "metal_tiny_remap", "plastic_ks_black"],
    "lambert": ["matte", "plastic_ks_black"],
    "rough_reflection": ["metal", "glass_kt_black"],
    "lambert_rough_reflection": ["matte", "plastic", "metal"],
    "rough_glass": ["glass_rough", "metal_aniso"],
    "mirror": ["mirror"],
    # more than kLdsMats (32) materials: production reads these templates from global memory
    "many": list(bq.MATERIALS) + ["matte"] * 15 + ["glass_aniso"],
}


@pytest.fixture(scope="module")
def hip():
    r = HipRenderer(0)
    yield r
    r.close()


def make_scene(names):
    s = scenes.Scene()
    for name in names:
        bq.add_material(s, name)
    P, I, UV = RS.uv_patch()
    s.mesh(P, I, 0, uv=UV)
    s.point_light((0.0, 3.0, 0.0), (10.0, 10.0, 10.0))
    return s


_frames = []


def hit_frames(hip):
    """(n, ns, dpdu) of a handful of pbr_hip_query hits on the uv patch (the scene must be uploaded)."""
    if not _frames:
        rays = np.array([[x, 2.0, z, 0.1 * x, -1.0, 0.05 * z, 1e30] for x, z in ((-2.1, 0.3), (0.4, -1.7), (1.3, 2.2), (2.2, -0.2))],
                        np.float32)
        for h in hip.query(rays):
            assert h.hit
            _frames.append((tuple(h.n), tuple(h.ns), tuple(h.dpdu)))
    return tuple(_frames)


def ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def transcendental_sample_rows(ls, q):
    """Rows whose sampled direction may come through sin / cos: a cosine lobe matches the type mask, or
    a microfacet lobe does and the stretched wo is within cos > .9999 of the normal (tr_sample11)."""
    rows = np.zeros(len(q), bool)
    wo = bx.Frame(q).to_local(q["wo"].astype(np.float64))
    for l in ls or ():
        m = bx._matches(l, q["type"])
        if l["kind"] in ("lambert", "oren"):
            rows |= m
        elif l["kind"] in ("mf_r", "mf_t"):
            ws = np.stack([l["ax"] * wo[:, 0], l["ay"] * wo[:, 1], np.abs(wo[:, 2])], -1)
            with np.errstate(invalid="ignore", divide="ignore"):
                rows |= m & ~(ws[:, 2] / np.linalg.norm(ws, axis=1) < 0.9999 - 1e-6)
    return rows


def compare_with_oracle(dev, ora, what, may_differ, counts, all_fields_transcendental=False):
    """Bit equality, with the transcendental allowance on the rows may_differ (the sample fields, or
    every field for a textured roughness).  counts: [rows on a transcendental path, rows that differed]."""
    differing = np.zeros(len(dev), bool)
    for fld in FIELDS:
        live = None
        if fld in ("s_wi", "d_wi"):
            live = dev["s_pdf" if fld == "s_wi" else "d_pdf"] != 0
        ne = bits_differ(dev, ora, fld, live)
        allowed = may_differ if (all_fields_transcendental or fld in SAMPLE_FIELDS) else np.zeros(len(dev), bool)
        bad = ne & ~allowed
        assert not bad.any(), f"{what}: {fld} differs on a path without a transcendental in {int(bad.sum())} queries, " \
                              f"first {int(np.argmax(bad))}: {dev[fld][np.argmax(bad)]} vs {ora[fld][np.argmax(bad)]}"
        if ne.any():
            assert dev[fld].dtype.kind == "f", f"{what}: {fld} differs"
            d = ulp_distance(dev[fld][ne], ora[fld][ne])
            assert d.max() <= 1, f"{what}: {fld} differs by {int(d.max())} ulp"
            differing |= ne
    counts[0] += int(may_differ.sum())
    counts[1] += int(differing.sum())


@pytest.mark.parametrize("scene_name", list(SCENES))
def test_device_equals_oracle_under_every_admissible_variant(hip, scene_name):
    names = SCENES[scene_name]
    s = make_scene(names)
    hip.upload(s)
    frames = hit_frames(hip)
    kinds = 0
    for name in names:
        kinds |= material_mask(name)
    variants = [v for v, mask in VARIANT_MASKS.items() if kinds & ~mask == 0]
    fits = 2 * len(names) <= 32
    if not fits:
        variants.remove(capi.BSDF_VARIANT_ALL_LDS)
    assert capi.BSDF_VARIANT_ALL in variants
    # (the duplicates that pad the large scene are queried at its last two indices only)
    indices = list(range(len(names))) if fits else list(range(len(bq.MATERIALS))) + [len(names) - 2, len(names) - 1]
    counts = [0, 0]
    for m in indices:
        for multi in (0, 1):
            q = bq.build(m, multi, extra_frames=frames)
            ora = oracle_lib.bsdf(s, q)
            ls = bx.lobes(names[m], multi)
            may = transcendental_sample_rows(ls, q)
            ref = hip.bsdf(q, capi.BSDF_VARIANT_ALL)
            compare_with_oracle(ref, ora, f"{scene_name}/{names[m]} multi={multi}", may, counts)
            assert_self_consistent(ref, f"{scene_name}/{names[m]} multi={multi}")
            for v in variants:
                if v == capi.BSDF_VARIANT_ALL:
                    continue
                dev = hip.bsdf(q, v)   # the lobe mask and the template source change no bit, d_ok included
                assert_records_equal(dev, ref, f"{scene_name}/{names[m]} multi={multi} variant {v} vs ALL", FIELDS + ("d_ok",))
    print(f"{scene_name}: variants {variants}; {counts[1]} of {counts[0]} transcendental-path queries differ from the oracle")
    assert counts[1] * 1000 <= counts[0], counts
    # a query past the materials has no BSDF; n = 1 and n = 0 launch
    q = bq.build(len(names), 1)[:1]
    assert hip.bsdf(q)["no_bsdf"][0] == 1 and hip.bsdf(bq.build(-1, 1)[:1])["no_bsdf"][0] == 1
    one = hip.bsdf(bq.build(0, 1)[:1])
    assert_records_equal(one, oracle_lib.bsdf(s, bq.build(0, 1)[:1]), "n = 1",
                         [f for f in FIELDS if f not in SAMPLE_FIELDS])
    assert len(hip.bsdf(bq.build(0, 1)[:0])) == 0


def textured_scene():
    """Per wrap mode: a matte with a Kd image texture and a plastic whose roughness is a float image
    texture remapped per hit (the device's log); mappings that send uv outside [0, 1]."""
    rng = np.random.default_rng(5)
    s = scenes.Scene()
    names = []
    for wrap in (capi.WRAP_REPEAT, capi.WRAP_BLACK, capi.WRAP_CLAMP):
        t_kd = s.image_texture(rng.uniform(0.05, 0.95, (5, 3, 3)).astype(np.float32), wrap=wrap, mapping=(1.3, 0.7, 0.2, -0.4))
        t_r = s.image_texture(np.repeat(rng.uniform(0.02, 0.6, (4, 6, 1)), 3, 2).astype(np.float32), is_float=True, wrap=wrap,
                              mapping=(0.9, 1.6, -0.3, 0.1))
        s.set_texture(s.matte((0.5, 0.5, 0.5)), capi.TEX_KD, t_kd)
        s.set_texture(s.plastic(kd=(0.3, 0.2, 0.1), ks=(0.6, 0.6, 0.6), rough=0.2, remap=True), capi.TEX_ROUGHNESS, t_r)
        names += ["matte_kd_texture", "plastic_roughness_texture"]
    P, I, UV = RS.uv_patch()
    s.mesh(P, I, 0, uv=UV)
    s.point_light((0.0, 3.0, 0.0), (10.0, 10.0, 10.0))
    return s, names


def test_textured_materials_equal_oracle(hip):
    s, names = textured_scene()
    hip.upload(s)
    counts = [0, 0]
    lambert = [dict(kind="lambert", type=bx.REFL | bx.DIFF)]
    for m, name in enumerate(names):
        for multi in (0, 1):
            q = bq.build(m, multi)
            ora = oracle_lib.bsdf(s, q)
            dev = hip.bsdf(q, capi.BSDF_VARIANT_TEXTURED)
            if name == "matte_kd_texture":   # the texture lookup is arithmetic: only the cosine sample reaches sin / cos
                compare_with_oracle(dev, ora, f"{name} {m} multi={multi}", transcendental_sample_rows(lambert, q), counts)
            else:                            # alpha comes through log: every field derives from it
                compare_with_oracle(dev, ora, f"{name} {m} multi={multi}", np.ones(len(q), bool), counts, True)
            assert_self_consistent(dev, f"{name} {m} multi={multi}")
            assert (dev["no_bsdf"] == 0).all() and (dev["pdf"] > 0).any()
    # a black-wrapped Kd outside the image has no lobe at all: some queries must see that, some not
    dev = hip.bsdf(bq.build(2, 1), capi.BSDF_VARIANT_TEXTURED)
    dead = (dev["pdf"] == 0) & (dev["s_pdf"] == 0)
    assert 0 < dead.sum() < len(dev)
    print(f"textured: {counts[1]} of {counts[0]} transcendental-path queries differ from the oracle")
    assert counts[1] * 1000 <= counts[0], counts
    # a textured scene may hold any lobe kind: every other variant is refused
    out = np.zeros(1, dtype=capi.bsdf_record_dtype())
    q = bq.build(0, 1)[:1]
    for v in VARIANT_MASKS:
        if v != capi.BSDF_VARIANT_TEXTURED:
            assert hip.lib.pbr_hip_bsdf(hip.ctx, v, 1, q.ctypes.data, out.ctypes.data) == capi.PBR_E_INVALID, v


def test_refusals(hip):
    out = np.zeros(1, dtype=capi.bsdf_record_dtype())
    q = bq.build(0, 1)[:1]
    qp, op = q.ctypes.data, out.ctypes.data
    fresh = HipRenderer(0)
    try:
        assert fresh.lib.pbr_hip_bsdf(fresh.ctx, capi.BSDF_VARIANT_ALL, 1, qp, op) == capi.PBR_E_NOSCENE
    finally:
        fresh.close()
    hip.upload(make_scene(SCENES["micro"]))
    lib = hip.lib
    for v in (capi.BSDF_VARIANT_SIMPLE, capi.BSDF_VARIANT_MATTE_MIRROR, capi.BSDF_VARIANT_MIRROR, capi.BSDF_VARIANT_PASS_L,
              capi.BSDF_VARIANT_PASS_R, capi.BSDF_VARIANT_PASS_LR, capi.BSDF_VARIANT_PASS_RT):
        assert lib.pbr_hip_bsdf(hip.ctx, v, 1, qp, op) == capi.PBR_E_INVALID, v
    for v in (-1, 13, 99):
        assert lib.pbr_hip_bsdf(hip.ctx, v, 1, qp, op) == capi.PBR_E_INVALID, v
    assert lib.pbr_hip_bsdf(hip.ctx, capi.BSDF_VARIANT_ALL, 1, None, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf(hip.ctx, capi.BSDF_VARIANT_ALL, 1, qp, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf(hip.ctx, capi.BSDF_VARIANT_ALL, -1, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf(None, capi.BSDF_VARIANT_ALL, 1, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_phase_hg(hip.ctx, 1, None, None) == capi.PBR_E_INVALID
    assert lib.pbr_hip_phase_hg(hip.ctx, -1, None, None) == capi.PBR_E_INVALID
    hip.upload(make_scene(SCENES["many"]))   # 34 materials: the templates do not fit the LDS copy
    assert lib.pbr_hip_bsdf(hip.ctx, capi.BSDF_VARIANT_ALL_LDS, 1, qp, op) == capi.PBR_E_INVALID
    assert lib.pbr_hip_bsdf(hip.ctx, capi.BSDF_VARIANT_ALL_GLOBAL, 1, qp, op) == capi.PBR_OK


def test_phase_hg_device_equals_oracle(hip):
    q = bq.build_phase()
    dev, ora = hip.phase_hg(q), oracle_lib.phase_hg(q)
    ne = (dev.view(np.uint32) != ora.view(np.uint32)) & ~(np.isnan(dev) & np.isnan(ora))
    # p(wo, wi) and the sampled direction's value reach no transcendental
    assert not ne[:, 0].any() and not ne[:, 4].any(), (int(ne[:, 0].sum()), int(ne[:, 4].sum()))
    rows = ne[:, 1:4].any(1)   # the direction comes through sin / cos of phi
    print(f"phase: {int(rows.sum())} of {len(q)} sampled directions differ from the oracle")
    if rows.any():
        assert ulp_distance(dev[:, 1:4][ne[:, 1:4]], ora[:, 1:4][ne[:, 1:4]]).max() <= 1
    assert rows.sum() * 1000 <= len(q), int(rows.sum())
    one = hip.phase_hg(q[:1])
    assert (one.view(np.uint32)[0, [0, 4]] == ora.view(np.uint32)[0, [0, 4]]).all()
    assert hip.phase_hg(q[:0]).shape == (0, 5)
