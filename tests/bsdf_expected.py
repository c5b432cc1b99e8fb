"""A float64 statement of the scattering functions the BSDF probe evaluates, written from the formulas
(Lambert, Oren-Nayar, Trowbridge-Reitz microfacet reflection and transmission, the Fresnel equations,
Snell's law, Henyey-Greenstein) and pbrt's BSDF-level rules — not from the float code's order of
operations.  It guards against an error the oracle and the device share.  The float32 inputs of a
query are taken as exact.  Vectorised over queries; test infrastructure only."""
import numpy as np

import bsdf_queries as bq
from pysicalbasedraytracer_amd import capi

REFL, TRANS, DIFF, GLOSSY, SPEC = (capi.BSDF_REFLECTION, capi.BSDF_TRANSMISSION, capi.BSDF_DIFFUSE, capi.BSDF_GLOSSY,
                                   capi.BSDF_SPECULAR)


def _f(x):
    """A float32 parameter as the exact float64 it denotes."""
    return np.asarray(np.asarray(x, np.float32), np.float64)


def roughness_to_alpha(r):
    x = np.log(np.maximum(r, 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x ** 2 + 0.0171201 * x ** 3 + 0.000640711 * x ** 4


def _alpha(r, remap):
    a = roughness_to_alpha(_f(r)) if remap else _f(r)
    return float(np.maximum(a, _f(0.001)))


def lobes(name, multi):
    """The BxDFs a material of bsdf_queries.MATERIALS adds (Material/*.cpp), float64 parameters."""
    method, kw = bq.MATERIALS[name]
    if method is None:
        return None
    out = []
    if method == "matte":
        R = np.clip(_f(kw["kd"]), 0, None)
        if R.any():
            sigma = float(np.clip(_f(kw["sigma"]), 0, 90))
            if sigma == 0:
                out.append(dict(kind="lambert", type=REFL | DIFF, R=R))
            else:
                s2 = np.radians(sigma) ** 2
                out.append(dict(kind="oren", type=REFL | DIFF, R=R, A=1 - s2 / (2 * (s2 + 0.33)), B=0.45 * s2 / (s2 + 0.09)))
    elif method == "mirror":
        R = np.clip(_f(kw["kr"]), 0, None)
        if R.any():
            out.append(dict(kind="spec_r", type=REFL | SPEC, R=R, fresnel=None))
    elif method == "glass":
        R, T = _f(kw.get("kr", (0.98,) * 3)), _f(kw.get("kt", (0.98,) * 3))
        eta, ur, vr = float(_f(kw["eta"])), kw["urough"], kw["vrough"]
        smooth = ur == 0 and vr == 0
        if not (R.any() or T.any()):
            return out
        if smooth and multi:
            return [dict(kind="fresnel_spec", type=REFL | TRANS | SPEC, R=R, T=T, etaA=1.0, etaB=eta)]
        remap = kw.get("remap", False)
        ax, ay = _alpha(ur, remap), _alpha(vr, remap)
        if R.any():
            out.append(dict(kind="spec_r", type=REFL | SPEC, R=R, fresnel=("diel", 1.0, eta)) if smooth else
                       dict(kind="mf_r", type=REFL | GLOSSY, R=R, fresnel=("diel", 1.0, eta), ax=ax, ay=ay))
        if T.any():
            out.append(dict(kind="spec_t", type=TRANS | SPEC, T=T, etaA=1.0, etaB=eta) if smooth else
                       dict(kind="mf_t", type=TRANS | GLOSSY, T=T, etaA=1.0, etaB=eta, ax=ax, ay=ay))
    elif method == "metal":
        remap = kw.get("remap", False)
        out.append(dict(kind="mf_r", type=REFL | GLOSSY, R=np.ones(3), ax=_alpha(kw["urough"], remap), ay=_alpha(kw["vrough"], remap),
                        fresnel=("cond", _f(kw.get("eta", (0.2, 0.2, 0.8))), _f(kw.get("k", (0.11, 0.11, 0.11))))))
    elif method == "plastic":
        kd = np.clip(_f(kw["kd"]), 0, None)
        ks = np.clip(_f(kw["ks"]) if "ks" in kw else _f(np.float32(1) - np.asarray(kw["kd"], np.float32)), 0, None)
        if kd.any():
            out.append(dict(kind="lambert", type=REFL | DIFF, R=kd))
        if ks.any():
            a = _alpha(kw["rough"], kw.get("remap", True))
            out.append(dict(kind="mf_r", type=REFL | GLOSSY, R=ks, fresnel=("diel", 1.5, 1.0), ax=a, ay=a))
    return out


# ---------------------------------------------------------------- Fresnel
def fr_dielectric(cos_i, eta_i, eta_t):
    """Unpolarised Fresnel reflectance at a dielectric boundary; cos_i < 0: incident from the eta_t side."""
    c = np.clip(np.asarray(cos_i, np.float64), -1, 1)
    ei = np.where(c > 0, eta_i, eta_t)
    et = np.where(c > 0, eta_t, eta_i)
    c = np.abs(c)
    st = ei / et * np.sqrt(1 - c * c)
    ct = np.sqrt(np.maximum(0, 1 - st * st))
    with np.errstate(invalid="ignore", divide="ignore"):
        rpar = (et * c - ei * ct) / (et * c + ei * ct)
        rper = (ei * c - et * ct) / (ei * c + et * ct)
    return np.where(st >= 1, 1.0, (rpar ** 2 + rper ** 2) / 2)


def fr_conductor(cos_i, eta, k):
    """Fresnel reflectance of a conductor of complex index eta + ik seen from vacuum, per channel."""
    c = np.clip(np.abs(np.asarray(cos_i, np.float64)), 0, 1)[..., None]
    n2 = (eta + 1j * k) ** 2
    root = np.sqrt(n2 - (1 - c * c))
    rs = (c - root) / (c + root)
    rp = (n2 * c - root) / (n2 * c + root)
    return (np.abs(rs) ** 2 + np.abs(rp) ** 2) / 2


def _fresnel(l, cos_i):
    fr = l.get("fresnel")
    if fr is None:
        return np.ones(np.shape(cos_i) + (3,))
    if fr[0] == "diel":
        return np.repeat(fr_dielectric(cos_i, fr[1], fr[2])[..., None], 3, -1)
    return fr_conductor(cos_i, fr[1], fr[2])


# ---------------------------------------------------------------- Trowbridge-Reitz
def _norm(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return np.sum(a * b, -1)


def tr_d(l, wh):
    """GGX normal distribution with anisotropic alphas."""
    ax, ay = l["ax"], l["ay"]
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1 / (np.pi * ax * ay * ((wh[..., 0] / ax) ** 2 + (wh[..., 1] / ay) ** 2 + wh[..., 2] ** 2) ** 2)


def tr_lambda(l, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (-1 + np.sqrt(1 + ((l["ax"] * w[..., 0]) ** 2 + (l["ay"] * w[..., 1]) ** 2) / w[..., 2] ** 2)) / 2


def _same_hemi(a, b):
    return a[..., 2] * b[..., 2] > 0


def _sin(w):
    return np.sqrt(np.maximum(0, 1 - w[..., 2] ** 2))


def _mf_t_half(l, wo, wi):
    eta = np.where(wo[..., 2] > 0, l["etaB"] / l["etaA"], l["etaA"] / l["etaB"])
    wh = _norm(wo + wi * eta[..., None])
    wh = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    return eta, wh


def lobe_f(l, wo, wi):
    """f(wo, wi) of one lobe, local directions [n, 3] → [n, 3]."""
    n = wo.shape[0]
    kind = l["kind"]
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "lambert":
            return np.broadcast_to(l["R"] / np.pi, (n, 3)).copy()
        if kind == "oren":
            si, so = _sin(wi), _sin(wo)
            ci, co = np.abs(wi[..., 2]), np.abs(wo[..., 2])
            # the azimuth term cos(phi_i - phi_o) is undefined at the normal: taken as 0 within 1e-4 of it
            cos_dphi = np.where((si > 1e-4) & (so > 1e-4), (wi[..., 0] * wo[..., 0] + wi[..., 1] * wo[..., 1]) / (si * so), 0)
            sin_alpha = np.maximum(si, so)                 # alpha: the larger polar angle
            tan_beta = np.minimum(si / ci, so / co)        # beta: the smaller
            return l["R"] / np.pi * (l["A"] + l["B"] * np.maximum(0, cos_dphi) * sin_alpha * tan_beta)[..., None]
        if kind == "mf_r":
            ci, co = np.abs(wi[..., 2]), np.abs(wo[..., 2])
            h = wi + wo
            dead = (ci == 0) | (co == 0) | (np.abs(h).sum(-1) == 0)
            wh = _norm(h)
            F = _fresnel(l, _dot(wi, np.where((wh[..., 2] < 0)[..., None], -wh, wh)))
            G = 1 / (1 + tr_lambda(l, wo) + tr_lambda(l, wi))
            f = l["R"] * F * (tr_d(l, wh) * G / (4 * ci * co))[..., None]
            return np.where(dead[..., None], 0.0, f)
        if kind == "mf_t":
            eta, wh = _mf_t_half(l, wo, wi)
            oh, ih = _dot(wo, wh), _dot(wi, wh)
            dead = _same_hemi(wo, wi) | (wi[..., 2] == 0) | (wo[..., 2] == 0) | (oh * ih > 0)
            F = fr_dielectric(oh, l["etaA"], l["etaB"])
            G = 1 / (1 + tr_lambda(l, wo) + tr_lambda(l, wi))
            # radiance transport: the eta^2 of the Jacobian cancels the 1 / eta^2 radiance scaling
            v = (1 - F) * tr_d(l, wh) * G * np.abs(ih) * np.abs(oh) / (np.abs(wi[..., 2] * wo[..., 2]) * (oh + eta * ih) ** 2)
            return np.where(dead[..., None], 0.0, l["T"] * v[..., None])
    return np.zeros((n, 3))   # specular lobes: f is a delta, 0 for given directions


def lobe_pdf(l, wo, wi):
    kind = l["kind"]
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind in ("lambert", "oren"):   # cosine-weighted hemisphere
            return np.where(_same_hemi(wo, wi), np.abs(wi[..., 2]) / np.pi, 0.0)
        if kind == "mf_r":   # visible normals: D G1(wo) |wo.wh| / |cos o|, times dwh/dwi = 1 / (4 wo.wh)
            wh = _norm(wo + wi)
            oh = _dot(wo, wh)
            p = tr_d(l, wh) / (1 + tr_lambda(l, wo)) * np.abs(oh) / np.abs(wo[..., 2]) / (4 * oh)
            return np.where(_same_hemi(wo, wi), p, 0.0)
        if kind == "mf_t":
            eta, wh = _mf_t_half(l, wo, wi)
            oh, ih = _dot(wo, wh), _dot(wi, wh)
            p = tr_d(l, wh) / (1 + tr_lambda(l, wo)) * np.abs(oh) / np.abs(wo[..., 2]) * np.abs(eta ** 2 * ih) / (oh + eta * ih) ** 2
            return np.where(_same_hemi(wo, wi) | (oh * ih > 0), 0.0, p)
    return np.zeros(wo.shape[0])


# ---------------------------------------------------------------- the BSDF level (Reflection.cpp:56-164)
class Frame:
    def __init__(self, q):
        self.ns, self.ng = q["ns"].astype(np.float64), q["n"].astype(np.float64)
        self.ss = _norm(q["dpdu"].astype(np.float64))
        self.ts = np.cross(self.ns, self.ss)

    def to_local(self, v):
        return np.stack([_dot(v, self.ss), _dot(v, self.ts), _dot(v, self.ns)], -1)

    def to_world(self, v):
        return v[..., 0:1] * self.ss + v[..., 1:2] * self.ts + v[..., 2:3] * self.ns


def _matches(l, flags):
    return (l["type"] & flags) == l["type"]


def bsdf_f(ls, q, wi_world=None):
    """BSDF::f: lobes matching the type mask, reflection or transmission lobes by the geometric normal."""
    fr = Frame(q)
    wo_w = q["wo"].astype(np.float64)
    wi_w = q["wi"].astype(np.float64) if wi_world is None else wi_world
    wo, wi = fr.to_local(wo_w), fr.to_local(wi_w)
    reflect = _dot(wi_w, fr.ng) * _dot(wo_w, fr.ng) > 0
    flags = q["type"]
    f = np.zeros((len(q), 3))
    for l in ls:
        use = _matches(l, flags) & np.where(reflect, (l["type"] & REFL) != 0, (l["type"] & TRANS) != 0)
        f += np.where(use[:, None], lobe_f(l, wo, wi), 0.0)
    return np.where((wo[:, 2] == 0)[:, None], 0.0, f)


def bsdf_pdf(ls, q, wi_world=None):
    """BSDF::Pdf: the mean over the lobes matching the type mask."""
    fr = Frame(q)
    wo = fr.to_local(q["wo"].astype(np.float64))
    wi = fr.to_local(q["wi"].astype(np.float64) if wi_world is None else wi_world)
    flags = q["type"]
    pdf, m = np.zeros(len(q)), np.zeros(len(q))
    for l in ls:
        use = _matches(l, flags)
        m += use
        pdf += np.where(use, lobe_pdf(l, wo, wi), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((m > 0) & (wo[:, 2] != 0), pdf / np.maximum(m, 1), 0.0)


def specular_sample(l, wo, reflect_branch=None):
    """Direction, weight f and pdf of a specular lobe's sample for local wo: (wi, f, pdf, type).
    fresnel_spec: reflect_branch says which of its two branches (its own pdf F or 1 - F)."""
    n = wo.shape[0]
    up = np.where(wo[:, 2:3] < 0, -1.0, 1.0) * np.array([0.0, 0, 1])   # the normal on wo's side

    def refl():
        return wo * np.array([-1.0, -1, 1])

    def refr():   # Snell: eta_i sin_i = eta_t sin_t, in the plane of incidence
        ei = np.where(wo[:, 2] > 0, l["etaA"], l["etaB"])
        et = np.where(wo[:, 2] > 0, l["etaB"], l["etaA"])
        eta = ei / et
        cos_i = np.abs(wo[:, 2])
        sin2_t = eta ** 2 * (1 - cos_i ** 2)
        cos_t = np.sqrt(np.maximum(0, 1 - sin2_t))
        wt = -eta[:, None] * wo + (eta * cos_i - cos_t)[:, None] * up
        return wt, sin2_t >= 1, (ei / et) ** 2

    with np.errstate(invalid="ignore", divide="ignore"):
        if l["kind"] == "spec_r":
            wi = refl()
            return wi, _fresnel(l, wi[:, 2]) * l["R"] / np.abs(wi[:, 2:3]), np.ones(n), np.full(n, l["type"])
        if l["kind"] == "spec_t":
            wi, tir, scale = refr()
            f = l["T"] * ((1 - fr_dielectric(wi[:, 2], l["etaA"], l["etaB"])) * scale / np.abs(wi[:, 2]))[:, None]
            return wi, np.where(tir[:, None], 0.0, f), np.where(tir, 0.0, 1.0), np.full(n, l["type"])
        F = fr_dielectric(wo[:, 2], l["etaA"], l["etaB"])
        wr = refl()
        wt, tir, scale = refr()
        fr_ = l["R"] * (F / np.abs(wr[:, 2]))[:, None]
        ft = np.where(tir[:, None], 0.0, l["T"] * ((1 - F) * scale / np.abs(wt[:, 2]))[:, None])
        rb = reflect_branch
        return (np.where(rb[:, None], wr, wt), np.where(rb[:, None], fr_, ft), np.where(rb, F, np.where(tir, 0.0, 1 - F)),
                np.where(rb, SPEC | REFL, SPEC | TRANS))


def phase_hg(cos_theta, g):
    """Henyey-Greenstein with pbrt's sign convention (cos_theta between wo and wi, both pointing away)."""
    return (1 - g * g) / (4 * np.pi * (1 + g * g + 2 * g * cos_theta) ** 1.5)


# ---------------------------------------------------------------- the conditioning rule
def ill_conditioned(ls, q, wi_world=None):
    """The queries left out of the float32 / float64 comparison, decided from the inputs alone:
    |cos theta| of wo or wi below 1e-3, |wo.wh| below 1e-3 for a microfacet lobe's half vector, or a
    dielectric Fresnel term evaluated within 1e-3 (in sin theta) of its critical angle, where the
    reflectance has a square-root singularity."""
    fr = Frame(q)
    wo = fr.to_local(q["wo"].astype(np.float64))
    wi = fr.to_local(q["wi"].astype(np.float64) if wi_world is None else wi_world)
    bad = (np.abs(wo[:, 2]) < 1e-3) | (np.abs(wi[:, 2]) < 1e-3)

    def critical(cos_i, a, b):
        return np.abs(np.sqrt(np.maximum(0, 1 - cos_i ** 2)) - min(a, b) / max(a, b)) < 1e-3

    with np.errstate(invalid="ignore", divide="ignore"):
        for l in ls or ():
            diel = l["fresnel"][1:] if (l.get("fresnel") or ("",))[0] == "diel" else None
            if l["kind"] == "mf_r":
                wh = _norm(wo + wi)
                bad |= ~(np.abs(_dot(wo, wh)) >= 1e-3)
                if diel:
                    bad |= critical(_dot(wi, wh), *diel)
            elif l["kind"] == "mf_t":
                _, wh = _mf_t_half(l, wo, wi)
                bad |= ~(np.abs(_dot(wo, wh)) >= 1e-3) | critical(_dot(wo, wh), l["etaA"], l["etaB"])
            elif l["kind"] == "spec_r" and diel:
                bad |= critical(wo[:, 2], *diel)
            elif l["kind"] in ("spec_t", "fresnel_spec"):
                bad |= critical(wo[:, 2], l["etaA"], l["etaB"])
    return bad
