// pbr_bsdf_probe.h — the scattering layer on caller-given directions (pbr_hip_bsdf, pbr_hip_phase_hg
// and their host twins): one query per lane through the BSDF functions of pbr_device.h, under the
// lobe mask K a production shading kernel is compiled with.  Test surface only: no render calls it.
//
// A separately compiled probe is not the production kernel.  The library is built with
// -ffp-contract=off, without fast-math and with correctly rounded fp32 division and square root, so
// every value is fixed by the source and the mask K, whichever kernel (or the host) evaluates it.
// Included by pbr_bsdf_probe.hip behind pbr_lobe_masks.h, in the same scope.
#pragma once

PBR_HD f3 ld_f3(const float* v) { return mk(v[0], v[1], v[2]); }
PBR_HD void st_f3(float* d, f3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
PBR_HD void st_rgb(float* d, rgb v) { d[0] = v.r; d[1] = v.g; d[2] = v.b; }

// One query.  mt: the material's lobe template as make_bsdf picks it (textures evaluated), or
// nullptr where make_bsdf returns false.  The frame is make_bsdf's.
template <int K>
PBR_HD void bsdf_probe_eval(const MatTemplate* mt, const pbr_bsdf_query& q, pbr_bsdf_record* out) {
    pbr_bsdf_record r;
    {
        int* w = (int*)&r;
        for (unsigned i = 0; i < sizeof(r) / 4; ++i) w[i] = 0;
    }
    if (!mt) {
        r.no_bsdf = 1;
        *out = r;
        return;
    }
    BSDF b;
    b.mt = mt;
    b.ns = ld_f3(q.ns);
    b.ng = ld_f3(q.n);
    b.ss = normalize(ld_f3(q.dpdu));
    b.ts = cross(b.ns, b.ss);
    const f3 wo = ld_f3(q.wo), wi = ld_f3(q.wi);
    st_rgb(r.f, bsdf_f<K>(b, wo, wi, q.type));
    r.pdf = bsdf_pdf<K>(b, wo, wi, q.type);
    const float lam = mf_lambda<K>(b, b.to_local(wo));   // as the Path and VolPath shades form it
    st_rgb(r.f_lam, bsdf_f_pdf<K>(b, wo, wi, q.type, &r.pdf_lam, lam));
    st_rgb(r.f_nolam, bsdf_f_pdf<K>(b, wo, wi, q.type, &r.pdf_nolam));
    {
        f3 swi = mk(0, 0, 0);
        float pdf = -1.f;
        int st = -1;
        st_rgb(r.s_f, bsdf_sample<K>(b, wo, &swi, q.u0, q.u1, &pdf, q.type, &st));
        st_f3(r.s_wi, swi);
        r.s_pdf = pdf;
        r.s_type = st;
    }
    {   // EstimateDirect's BSDF sample (pbr_wavefront_path.h estimate_bsdf_sample): the direction, then the sum
        f3 swi = mk(0, 0, 0);
        float pdf = -1.f;
        int st = -1;
        BsdfDraw draw;
        const bool ok = bsdf_sample_dir<K>(b, wo, &swi, q.u0, q.u1, &pdf, q.type, &st, &draw, lam);
        if (ok) st_rgb(r.d_f, bsdf_sample_sum<K>(b, wo, swi, q.type, draw));
        st_f3(r.d_wi, swi);
        r.d_pdf = pdf;
        r.d_type = st;
        r.d_ok = ok ? 1 : 0;
    }
    *out = r;
}

// queries: g, wo.xyz, wi.xyz, u0, u1; out: p(wo, wi), sampled wi.xyz, its value
PBR_HD void phase_probe_eval(const float* q, float* o) {
    const float g = q[0];
    const f3 wo = ld_f3(q + 1), wi = ld_f3(q + 4);
    o[0] = phase_hg(dot(wo, wi), g);   // HenyeyGreenstein::p (Medium.cpp:5-7)
    f3 swi = mk(0, 0, 0);
    o[4] = hg_sample(g, wo, &swi, q[7], q[8]);
    st_f3(o + 1, swi);
}

#if defined(__HIPCC__) || defined(__HIP__)
// MATS_LDS / TEX: where a production kernel of this mask reads the templates (stage_mats, make_bsdf<TEX>)
template <int K, bool MATS_LDS, bool TEX>
__global__ void __launch_bounds__(256) k_bsdf_probe(DeviceScene S, int n, const pbr_bsdf_query* queries, pbr_bsdf_record* out) {
    const MatTemplate* mats = stage_mats<MATS_LDS>(S);
    if constexpr (MATS_LDS) __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const pbr_bsdf_query q = queries[i];
    MatTemplate texLocal;   // a textured material's per-hit lobes (make_bsdf)
    const MatTemplate* mt = nullptr;
    if (q.material >= 0 && q.material < S.nMaterials) {   // make_bsdf, with the material given instead of a hit's
        mt = mats + 2 * q.material + (q.multi_lobe ? 1 : 0);
        if (!mt->valid) mt = nullptr;
        else if constexpr (TEX) {
            if (mt->textured) {
                textured_template(S.texMats, S.textures, S.texels, q.material, q.uv[0], q.uv[1], q.multi_lobe != 0, &texLocal);
                mt = &texLocal;
            }
        }
    }
    bsdf_probe_eval<K>(mt, q, out + i);
}

__global__ void __launch_bounds__(256) k_phase_probe(int n, const float* queries, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float q[9], o[5];
    for (int k = 0; k < 9; ++k) q[k] = queries[(size_t)9 * i + k];
    phase_probe_eval(q, o);
    for (int k = 0; k < 5; ++k) out[(size_t)5 * i + k] = o[k];
}
#endif
