// pbr_wavefront_volpath.h — wavefront schedule for VolPathIntegrator::Li (VolPathIntegrator.cpp:
// 21-107) over homogeneous media.  Included after pbr_wavefront_path.h; shares its queues, camera
// kernel, probe kernel (the BSDF/phase-sampled ray of EstimateDirect is a plain Scene::Intersect,
// Integrator.cpp:159) and finish.  Differences from the Path schedule:
//   * rays carry their medium (packed into the queue's dim word);
//   * every bounce first samples the ray's medium (HomogeneousMedium::Sample, two Get1D), which can
//     turn the bounce into a medium interaction (HG phase function instead of a BSDF);
//   * the light sample's visibility is VisibilityTester::Tr (Light.cpp:31-47): k_wfv_tr walks the
//     shadow ray through medium interfaces, multiplying homogeneous transmittance, and the
//     resolve multiplies Li by it before the !IsBlack test, in the reference's op order.
#pragma once

constexpr int kWfvDelta = 8;   // dFlags: the estimate's light is a delta light

struct WfvParams {
    WfpParams X;
    // transmittance-walk queue (segmented): origin+tMax, dir + medium, target p, pError, n, the
    // direct record it fills
    float4* to; float4* td; float4* tp; float4* te; float4* tn; int* tid; int* trSeg;
    // direct records (at the direct queue position, like WfpParams' d*)
    float4* dLiA;          // light sample Li.rgb, lightPdf
    float4* dTr;           // transmittance to the light sample
    float* dWA;            // MIS weight of the light sample
    int anyHitTr;          // every primitive has a material: the walk is one any-hit query
};

// Waves per SIMD (C5: 2 → 1940 ms, 3 → 1832-1846, 4 → 1898)
#ifndef PBR_WFV_OCC
#define PBR_WFV_OCC 3
#endif
// The material pass of a queued VolPath ray (the classed shade): a ray inside a medium goes to pass
// 0, as do misses and material-less hits; a ray outside media goes to its hit material's pass.
// Pass 0 is the medium pass (k_wfv_shade<0, …, CLASSED>: no BSDF lobes): it samples the medium of
// every ray inside one and shades the medium events; a ray that reaches a surface with a material
// instead leaves its state after the medium sample (β, the sampler dimension) in its queue entry
// and is filed, flagged kDeferred, into that material's pass, which continues it from there.
__device__ __forceinline__ int entry_pass_vol(const WfpParams& X, int q) {
    if (((__float_as_int(X.W.cur.d[q].w) >> 24) & 0xff) != 0) return 0;   // in a medium (pack_path)
    return entry_pass(X, q);
}
// One bounce of VolPathIntegrator::Li for every queued ray: k_wfp_shade's steps around the medium
// sample, with the phase function in place of the BSDF at a medium event.  The light sample's f,
// Li, pdf and weight stay apart in the record, because the resolve multiplies Li by the walk's
// transmittance first.  (Template parameters: documented at k_wfp_shade.)
template <bool NRM, int LOBES, bool MATS_LDS, int OCC = PBR_WFV_OCC, int SMP = -1, bool CLASSED = false>
__global__ __launch_bounds__(256, OCC) void k_wfv_shade(WfvParams V, int level0, int pass) {
    constexpr bool kMediumPass = CLASSED && LOBES == 0;   // pass 0 of the classed shade
    WfpParams& X = V.X;
    WfParams& W = X.W;
    const KParams& P = W.P;
    const DeviceScene& S = P.S;
    stage_halton_lds(P.smp);
    const MatTemplate* mats = stage_mats<MATS_LDS>(S);
    __shared__ int s_push[4];   // transmittance walk, probe, direct, next (shade_entries)
    const int base = wf_block() * W.segCap;
    // One queued ray.  deferredIn: the medium pass left this entry after its medium sample.
    // Returns the pass a medium-pass entry is deferred to (0: shaded here).
    auto shade = [&](const bool active, const int q, const bool deferredIn) -> int {
        // Two phases around the light-estimate pushes: the record, the transmittance walk and the
        // probe ray are written before the path's phase-function / BSDF sample.
        bool pushNext = false;
        PathEntry e;
        Ray cont;
        Isect isect;   // the surface hit, or the medium interaction once one is sampled
        BSDF bsdf;
        MatTemplate texLocal;   // a textured material's per-hit lobes (make_bsdf)
        bool estimate = false, mediumEvent = false;
        float g = 0;
        bool pushDirect;
        int di;
        int deferTo = 0;
        {
            bool pushTr = false, pushProbe = false;
            Ray shadow, probe;
            VisPt vis;
            DirectRec rec;
            rgb Li;
            float weightA = 0.f, lightPdf = 0.f;
            if (active) {
                load_entry(W, q, level0, level0 && !deferredIn, &e);
                const Ray& ray = e.ray;
                const bool found = e.hit.slot >= 0;
                if (found) {
                    hit_isect<NRM>(S, e.hit, ray, &isect);
                    set_interface(S, &isect, ray.medium);
                }
                // HomogeneousMedium::Sample (HomogeneousMedium.cpp:15-45)
                if (ray.medium >= 0 && !deferredIn) {
                    const float* md = S.media + 10 * ray.medium;
                    int channel = (int)(get1d<true, SMP>(P.smp, e.st) * 3);
                    if (channel > 2) channel = 2;
                    float dist = -t_log(1 - get1d<true, SMP>(P.smp, e.st)) / md[6 + channel];
                    float t = mn(dist / len(ray.d), ray.tMax);
                    bool sampled = t < ray.tMax;
                    if (sampled) {
                        // MediumInteraction: it replaces the surface record, which a medium event never
                        // reads again (one record, no pointer select between two: that kept both in scratch)
                        isect.p = ray.o + ray.d * t; isect.wo = -ray.d; isect.n = mk(0, 0, 0); isect.pError = mk(0, 0, 0);
                        isect.sn = mk(0, 0, 0); isect.dpdu = mk(0, 0, 0);
                        isect.medIn = isect.medOut = ray.medium; isect.slot = -1;
                        g = md[9];
                        mediumEvent = true;
                    }
                    rgb Tr = exp_s(sp3(-md[6], -md[7], -md[8]) * mn(t, kMaxFloat) * len(ray.d));
                    rgb density = sampled ? (sp3(md[6], md[7], md[8]) * Tr) : Tr;
                    float pdf = 0;
                    pdf += density.r; pdf += density.g; pdf += density.b;
                    pdf *= 1 / (float)3;
                    if (pdf == 0) pdf = 1;
                    e.beta = e.beta * (sampled ? (Tr * sp3(md[3], md[4], md[5]) / pdf) : (Tr / pdf));
                }
                if constexpr (kMediumPass) {
                    // a surface with a material reached from inside the medium: its material's pass
                    // continues the path from the state after the medium sample
                    if (ray.medium >= 0 && !mediumEvent && found) {
                        const int mat = S.primInfo[e.hit.slot].y;
                        if (mat >= 0 && mats[2 * mat + 1].valid) deferTo = X.matPass[mat];
                    }
                    if (deferTo > 0) {
                        W.cur.d[q] = make_float4(ray.d.x, ray.d.y, ray.d.z,
                                                 __int_as_float(pack_path(e.st.dim, e.bounces, e.specularBounce, ray.medium)));
                        W.cur.s0[q] = make_float4(e.L.r, e.L.g, e.L.b, e.beta.r);
                        W.cur.s1[q] = make_float4(e.beta.g, e.beta.b, e.etaScale, __uint_as_float(e.st.index));
                    }
                }
                bool alive = deferTo == 0 && !black(e.beta);
                if (alive && mediumEvent) {
                    if (e.bounces >= P.maxDepth) alive = false;
                    else estimate = true;
                } else if (alive) {
                    add_emission(S, isect, &e);
                    if (!found || e.bounces >= P.maxDepth) alive = false;
                    else if (!make_bsdf<(LOBES & kTexturedLobes) != 0>(S, mats, isect, true, &bsdf, &texLocal)) {
                        cont = spawn_ray(isect, ray.d);   // bounces--; continue: no Russian roulette
                        pushNext = true;
                        alive = false;
                    } else {
                        estimate = true;
                    }
                }
                if (estimate && S.nLights > 0) {
                    // UniformSampleOneLight(handleMedia = true) / EstimateDirect
                    const int li = sample_light(S, get1d<true, SMP>(P.smp, e.st), &rec.pmf);
                    if (rec.pmf != 0) {
                        float uL0, uL1, uS0, uS1;
                        get2d<true, SMP>(P.smp, e.st, &uL0, &uL1);
                        get2d<true, SMP>(P.smp, e.st, &uS0, &uS1);
                        const DLight& light = S.lights[li];
                        const bool delta = light.type == LT_POINT;
                        const int flagsNS = BSDF_ALL & ~BSDF_SPECULAR;
                        rec.flags = delta ? kWfvDelta : 0;
                        f3 wi = mk(0, 0, 0);
                        // Lambda(wo) of the microfacet lobes, once for the estimate's two strategies
                        const float lamL = mediumEvent ? kNoLambda : mf_lambda<LOBES>(bsdf, bsdf.to_local(isect.wo));
                        Li = sample_li<NRM>(S, light, isect, uL0, uL1, &wi, &lightPdf, &vis);
                        rec.a = sp(0.f);
                        if (lightPdf > 0 && !black(Li)) {
                            if (!mediumEvent) rec.a = bsdf_f_pdf<LOBES>(bsdf, isect.wo, wi, flagsNS, &rec.scatPdf, lamL) * absdot(wi, isect.sn);
                            else rec.a = sp(phase_hg(dot(isect.wo, wi), g));
                            if (!black(rec.a)) {
                                float fp = 1 * lightPdf, gp = 1 * rec.scatPdf;
                                weightA = (fp * fp) / (fp * fp + gp * gp);
                                shadow = spawn_ray_to(isect, vis.p, vis.pError, vis.n);
                                pushTr = true;
                                rec.flags |= kWfpAPending;
                            }
                        }
                        rec.fB = sp(0.f);
                        if (!delta && !mediumEvent) {
                            pushProbe = estimate_bsdf_sample<LOBES, NRM>(S, light, bsdf, isect, uS0, uS1, lamL, &rec, &probe);
                        } else if (!delta) {   // the phase function's sample: its value is its pdf
                            const float p = hg_sample(g, isect.wo, &wi, uS0, uS1);
                            rec.fB = sp(p);
                            rec.scatPdf = p;
                            if (!black(rec.fB) && p > 0) {
                                const float lp = pdf_li<NRM>(S, light, isect, wi);
                                if (lp != 0) {
                                    float fp = 1 * p, gp = 1 * lp;
                                    rec.weightB = (fp * fp) / (fp * fp + gp * gp);
                                    probe = spawn_ray(isect, wi);
                                    pushProbe = true;
                                }
                            }
                        }
                        if (pushProbe) rec.flags |= kWfpBPending;
                        rec.light = li;
                    }
                }
            }
            pushDirect = rec.pending();
            di = push_direct(X, &s_push[2], base, rec, e.beta);
            if (pushDirect) {
                V.dLiA[di] = make_float4(Li.r, Li.g, Li.b, lightPdf);
                V.dWA[di] = weightA;
            }
            const int ti = base + wave_push(&s_push[0], pushTr);
            if (pushTr) {
                V.to[ti] = make_float4(shadow.o.x, shadow.o.y, shadow.o.z, shadow.tMax);
                V.td[ti] = make_float4(shadow.d.x, shadow.d.y, shadow.d.z, __int_as_float(shadow.medium));
                if (!V.anyHitTr) {   // the walk's target; one any-hit query needs none of it
                    V.tp[ti] = make_float4(vis.p.x, vis.p.y, vis.p.z, 0.f);
                    V.te[ti] = make_float4(vis.pError.x, vis.pError.y, vis.pError.z, 0.f);
                    V.tn[ti] = make_float4(vis.n.x, vis.n.y, vis.n.z, 0.f);
                }
                V.tid[ti] = di;
            }
            push_probe(X, &s_push[1], base, pushProbe, probe, di);
        }
        if (estimate) {
            bool goesOn;
            if (mediumEvent) {   // HenyeyGreenstein::Sample_p, then the ray leaves the interaction
                f3 wo = -e.ray.d, wi;
                float u0, u1;
                get2d<true, SMP>(P.smp, e.st, &u0, &u1);
                hg_sample(g, wo, &wi, u0, u1);
                cont = spawn_ray(isect, wi);
                e.specularBounce = false;
                goesOn = true;
            } else {
                goesOn = sample_bounce<LOBES, SMP>(P, bsdf, isect, &e, &cont);
            }
            if (goesOn && survives_roulette<SMP>(P, &e)) {
                pushNext = true;
                e.bounces += 1;
            }
        }
        push_next(X, &s_push[3], base, active && deferTo == 0, pushNext, e, cont, cont.medium, pushDirect, di);
        return deferTo;
    };
    shade_entries<CLASSED, kMediumPass>(X, V.trSeg, s_push, level0, pass, [&](int q) { return entry_pass_vol(X, q); }, shade);
}

// VisibilityTester::Tr (Light.cpp:31-47): walk to the light sample through medium interfaces.
// Its lane-refill walk fetches near/far plane rows (PBR_NF_ROWS) although that spills 9 VGPRs here:
// C5 transmittance 340.8 ms/frame without the rows, 327.3 with them at 5 workgroups per CU (no
// spill), 321.5 with them at 6 (kept; serial schedule, profiles/r6_ab_tr.log).
// The transmittance of walk q when every surface has a material: the walk's first hit, if any,
// returns 0 and a miss multiplies the medium's Tr over the unchanged ray, so whether anything is
// hit is all that matters, and IntersectP answers that (same boolean, same ray on a miss).
__device__ __forceinline__ void tr_any_hit_result(const WfvParams& V, int q, bool hit, const Ray& ray) {
    rgb Tr = sp(1.f);
    if (hit) Tr = sp(0.0f);
    else if (ray.medium >= 0) Tr = Tr * medium_tr(V.X.W.P.S, ray.medium, ray);
    V.dTr[V.tid[q]] = make_float4(Tr.r, Tr.g, Tr.b, 0.f);
}

template <int SHORT>
__global__ __launch_bounds__(256, PBR_REFILL_OCC_TR) void k_wfv_tr(WfvParams V) {
    WfpParams& X = V.X;
    const DeviceScene& S = X.W.P.S;
    const int n = seg_scan(V.trSeg);
    if constexpr (kRefill > 0 && SHORT > 0 && kQuadTraversal) {
        if (V.anyHitTr) {   // lane-refill traversal
            traverse_stream<true, SHORT>(   // (not kAnyShort: see pbr_device.h)
                S, n, X.W.segCap,
                [&](int q, int* key) {
                    *key = q;
                    const float4 o = V.to[q], d = V.td[q];
                    return mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, __float_as_int(d.w));
                },
                [&](int q, bool hit, const Ray& ray, const HitRec&) { tr_any_hit_result(V, q, hit, ray); },
                X.W.prof, KP_WFV_TR);
            return;
        }
    }
    for (int i0 = wf_block() * blockDim.x + ((int)threadIdx.x & ~63); i0 < n; i0 += gridDim.x * blockDim.x) {   // per wave
        const int i = i0 + (int)__lane_id();
        const int q = seg_pos_dense(X.W.segCap, i, n);
        if (i >= n) continue;
        const float4 o = V.to[q], d = V.td[q];
        Ray ray = mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, __float_as_int(d.w));
        if (V.anyHitTr) {
            HitRec h;
            Counters c;
            tr_any_hit_result(V, q, traverse<true, false, SHORT>(S, ray, &h, &c), ray);
            continue;
        }
        const float4 tp = V.tp[q], te = V.te[q], tn = V.tn[q];
        const f3 p1 = mk(tp.x, tp.y, tp.z), e1 = mk(te.x, te.y, te.z), n1 = mk(tn.x, tn.y, tn.z);
        rgb Tr = sp(1.f);
        for (int guard = 0;; ++guard) {
            HitRec h;
            Counters c;
            const bool hit = traverse<false, false, SHORT>(S, ray, &h, &c);
            if (hit && S.primInfo[h.slot].y >= 0) { Tr = sp(0.0f); break; }
            if (ray.medium >= 0) Tr = Tr * medium_tr(S, ray.medium, ray);
            if (!hit) break;
            if (guard == kMaxTrCrossings) { atomicOr(S.guard, kGuardTransmittance); break; }
            Isect isect;
            hit_isect(S, h, ray, &isect);
            set_interface(S, &isect, ray.medium);
            ray = spawn_ray_to(isect, p1, e1, n1);
        }
        V.dTr[V.tid[q]] = make_float4(Tr.r, Tr.g, Tr.b, 0.f);
    }
}

// Ld = [f·(Li·Tr)·w/lightPdf if Li·Tr is not black] + [f·Li·w/scatteringPdf if Li is not black];
// L += beta · (Ld / pmf)
__global__ __launch_bounds__(256) void k_wfv_resolve(WfvParams V) {
    WfpParams& X = V.X;
    const int n = seg_scan(X.directSeg);
    for (int i0 = wf_block() * blockDim.x + ((int)threadIdx.x & ~63); i0 < n; i0 += gridDim.x * blockDim.x) {   // per wave
        const int i = i0 + (int)__lane_id();
        const int di = seg_pos_dense(X.W.segCap, i, n);
        if (i >= n) continue;
        const int fl = X.dFlags[di];
        const float4 a = X.dA[di], bt = X.dBeta[di];
        rgb Ld = sp(0.f);
        if (fl & kWfpAPending) {
            const float4 la = V.dLiA[di], tr = V.dTr[di];
            const rgb Lt = sp3(la.x, la.y, la.z) * sp3(tr.x, tr.y, tr.z);
            if (!black(Lt)) {
                const rgb fA = sp3(a.x, a.y, a.z);
                if (fl & kWfvDelta) Ld = Ld + fA * Lt / la.w;
                else Ld = Ld + fA * Lt * V.dWA[di] / la.w;
            }
        }
        if (fl & kWfpBPending) {
            const float4 li = X.dLi[di], b = X.dB[di];
            const rgb Li2 = sp3(li.x, li.y, li.z);
            if (!black(Li2)) Ld = Ld + sp3(b.x, b.y, b.z) * Li2 * b.w / bt.w;
        }
        const rgb beta = sp3(bt.x, bt.y, bt.z);
        add_direct(X, X.dTgt[di], beta * (Ld / a.w));
    }
}
