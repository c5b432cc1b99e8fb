// pbr_wavefront_path.h — wavefront schedule for PathIntegrator::Li (PathIntegrator.cpp:32-110) with
// UniformSampleOneLight / EstimateDirect (Integrator.cpp:46-177).  Included by pbr_kernels.hip
// after pbr_wavefront.h (queues, segment scan, wave_push, the camera/extend kernels).
//
// Per bounce k:
//   k_wfp_shade    emission (bounce 0 / after specular), BSDF, the one-light estimate's two
//                  candidate terms — light sample (needs a shadow ray) and BSDF sample (needs a
//                  probe ray) — and the continuation (BSDF sample, beta update, Russian roulette)
//   k_wfp_shadow   any-hit for the light-sample rays → "visible" flag in the direct record
//   k_wfp_probe    closest hit for the BSDF-sample rays → the radiance the sampled light shows there
//   k_wfp_resolve  Ld = [A if visible] + [f·Li·weight/scatteringPdf]; L += beta · (Ld / pmf)
//   k_wf_extend    closest hit for the continuation queue (shared with Whitted)
// then k_wfp_finish sums each pixel's per-sample L in sample order and runs the film.
//
// The path state — L, beta, etaScale and the sample's global index — travels with the ray in the
// queues (WfQueue s0/s1, compacted with the ray), and the direct-light estimate of bounce k is a
// record at its own position of the direct queue, which the shadow/probe entries point at: every
// kernel reads and writes its queue entries densely instead of gathering per-sample state by
// sample id from a compacted queue (which moved 3.5-8x the algorithmic bytes: partial lines).
// A path's L leaves the queues once, when the path ends (stL[id], read by the finish).  The
// estimate's record names where L is at resolve time — the continuation entry the same shade
// pushed, or stL[id] — and resolve adds the direct term there.  Every L update therefore happens
// in the reference's order (emission of bounce k, direct light of bounce k, emission of bounce
// k+1, ...), so the per-sample radiance is bit-identical to the recursive megakernel's.  Sampler
// dimensions travel in the ray queue.
#pragma once

constexpr int kWfpAPending = 1, kWfpBPending = 2, kWfpVisible = 4;

struct WfpParams {
    WfParams W;            // queues (cur/next rays with the path state, shadow), chunk geometry, sample index table
    // probe queue (segmented): origin+tMax, dir, the direct record it fills
    float4* po; float4* pd; int* pid; int* probeSeg;
    int* directSeg;        // direct-light records, segmented like the queues (at the shade's push position)
    float4* stL;           // the finished path's L.rgb, per sample (the finish's input)
    float4* dA;            // light-sample term f·Li·w/lightPdf (if unoccluded), pmf
    float4* dB;            // BSDF-sample f (× |cos|), weight
    float4* dBeta;         // beta at the estimate, scatteringPdf
    float4* dLi;           // probe result: Li at the BSDF-sampled direction
    int* dFlags;           // kWfp* bits
    int* dLight;           // light index of the estimate
    int* dTgt;             // where the path's L is when the estimate resolves: the continuation's
                           // position in the next queue, or ~id (stL[id]) when the path ended
    int lastLevel;         // this shade is the schedule's last: a continuation ends the path instead
    const int* matPass;    // the classed shade (CLASSED): the pass that shades each material's hits
    int* passList;         // ... the queue positions of passes 1.. ([pass - 1][segmented], filed by pass 0)
    int* passCnt;          // ... their counts ([pass - 1][workgroup])
    int passStride;        // ... entries per pass list
    int nPasses;
};

// The material pass of a queued hit (the classed shade): misses and material-less hits go to pass 0.
__device__ __forceinline__ int entry_pass(const WfpParams& X, int q) {
    const int slot = __float_as_int(X.W.cur.hit[q].x);
    if (slot < 0) return 0;
    const int mat = X.W.P.S.primInfo[slot].y;
    return mat < 0 ? 0 : X.matPass[mat];
}

// A queued ray's dim word: the sampler dimension, the bounce count, "the bounce before was
// specular", and the ray's medium (VolPath; -1: none, as every Path ray).
__device__ __forceinline__ int pack_path(int dim, int bounces, bool specular, int medium) {
    return (dim & 0xffff) | ((bounces & 0x7f) << 16) | (specular ? (1 << 23) : 0) | ((medium + 1) << 24);
}

template <int SHORT, bool PASS = false>
__global__ __launch_bounds__(256, PBR_TRAV_OCC) void k_wfp_camera_extend(WfpParams X) {
    WfParams& W = X.W;
    const KParams& P = W.P;
    int q = wf_block() * blockDim.x + threadIdx.x;
    if (q >= W.nSamples) return;
    int lp = q / P.spp, s = q - lp * P.spp;
    int x, y;
    pixel_xy(P, W.chunkPix0 + lp, &x, &y);
    SState st;
    st.index = sample_index(P.smp, x, y, PASS ? P.smp.passFirst + s : s).lo;
    st.sid = s;
    st.dim = 0;
    st.px = x;
    st.py = y;
    Ray r = camera_sample_ray(P, st, x, y);
    HitRec h;
    Counters c;
    bool hit;
    if constexpr (kPacket && kQuadTraversal) {   // a wave holds (part of) one pixel's samples
        h.slot = -1; h.b0 = h.b1 = h.b2 = 0.f;
        hit = traverse_wave<false>(P.S, r, &h, true);
    } else {
        hit = traverse<false, false, SHORT>(P.S, r, &h, &c);
    }
    trav_diag(W.prof, KP_WFP_CAMERA, h);
    W.cur.o[q] = make_float4(r.o.x, r.o.y, r.o.z, r.tMax);
    W.cur.d[q] = make_float4(r.d.x, r.d.y, r.d.z, __int_as_float(pack_path(st.dim, 0, false, -1)));
    W.cur.hit[q] = make_float4(__int_as_float(hit ? h.slot : -1), h.b0, h.b1, h.b2);
    W.sampleIndex[q] = st.index;   // the level-0 state (L = 0, beta = 1, etaScale = 1) is implied
}

// (A workgroup-local stable sort of each iteration's 256 shading events by miss / medium / material
// before shading was measured and removed: bit-identical, but C4 7711 → 7865 ms, C5 1373 → 1429,
// C3 269.7 → 270.8 — its barriers and key loads cost more than the divergence they removed.)

// ---- The steps of one bounce that PathIntegrator::Li and VolPathIntegrator::Li share.  Each takes
// what it needs and is called from inside the `shade` lambda of k_wfp_shade and of k_wfv_shade.

// A queue entry, unpacked: the ray, its hit, and the path state that travels with it.
struct PathEntry {
    Ray ray;
    HitRec hit;                   // slot < 0: the ray escaped
    int id = 0, bounces = 0;
    bool specularBounce = false;
    rgb L, beta;
    float etaScale = 1.f;
    SState st = {0, 0, 0, 0, 0};  // the sample's index and the next sampler dimension
};

// fresh: a camera ray's entry, whose state (L = 0, beta = 1, etaScale = 1) is implied
__device__ __forceinline__ void load_entry(const WfParams& W, int q, bool level0, bool fresh, PathEntry* e) {
    const float4 o = W.cur.o[q], d = W.cur.d[q], hr = W.cur.hit[q];
    e->id = level0 ? q : W.cur.id[q];
    const int dd = __float_as_int(d.w);   // pack_path
    e->bounces = (dd >> 16) & 0x7f;
    e->specularBounce = (dd >> 23) & 1;
    e->ray = mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, ((dd >> 24) & 0xff) - 1);
    e->hit = HitRec{__float_as_int(hr.x), hr.y, hr.z, hr.w};
    if (fresh) {
        e->L = sp(0.f); e->beta = sp(1.f); e->etaScale = 1.f;
        e->st.index = W.sampleIndex[q];
    } else {
        const float4 a = W.cur.s0[q], b = W.cur.s1[q];
        e->L = sp3(a.x, a.y, a.z); e->beta = sp3(a.w, b.x, b.y);
        e->etaScale = b.z;
        e->st.index = __float_as_uint(b.w);
    }
    e->st.sid = e->id;   // ≡ the sample number mod spp (pixel-major ids)
    e->st.dim = dd & 0xffff;
}

// Emission the path sees itself: at the camera ray's end and after a specular bounce (the light
// estimate of the bounce before accounts for it otherwise)
__device__ __forceinline__ void add_emission(const DeviceScene& S, const Isect& isect, PathEntry* e) {
    if (!(e->bounces == 0 || e->specularBounce)) return;
    if (e->hit.slot >= 0) e->L = e->L + e->beta * si_Le(S, isect, -e->ray.d);
    else for (int k = 0; k < S.nInfinite; ++k) e->L = e->L + e->beta * light_Le(S, S.lights[S.infinite[k]], e->ray);
}

// A direct-light estimate (UniformSampleOneLight / EstimateDirect) that waits for its rays: what the
// shade leaves for the resolve at the direct queue's next position.
struct DirectRec {
    rgb a;                 // the light sample's term: Path f·Li·w/lightPdf, VolPath f alone (Li, the
                           // pdf and the weight wait for the transmittance in records of its own)
    rgb fB;                // the BSDF (phase) sample's f·|cos|
    float weightB = 1.f, scatPdf = 0.f, pmf = 0.f;
    int flags = 0, light = 0;
    __device__ bool pending() const { return (flags & (kWfpAPending | kWfpBPending)) != 0; }
};

// EstimateDirect's BSDF sample (Integrator.cpp:126-174) at a surface, for a light that is not a
// delta light: fills r->fB, weightB and scatPdf; true: *probe has to find out what the light shows
// along the sampled direction.  The sample's value f·|cos| is only read when the sampled direction
// can reach the light — a specular sample, or Pdf_Li != 0 — so it is formed only then (the checks
// are pure, so their order does not change the outcome): most sampled directions miss a small area
// light and skip the sum over the lobes.
template <int LOBES, bool NRM = true>
__device__ __forceinline__ bool estimate_bsdf_sample(const DeviceScene& S, const DLight& light, const BSDF& bsdf, const Isect& isect,
                                                     float u0, float u1, float lamL, DirectRec* r, Ray* probe) {
    if constexpr ((PBR_DIAG_SHADE & 2) != 0) return false;
    const int flagsNS = BSDF_ALL & ~BSDF_SPECULAR;
    f3 wi = mk(0, 0, 0);
    int stype = 0;
    BsdfDraw draw;
    if (!bsdf_sample_dir<LOBES>(bsdf, isect.wo, &wi, u0, u1, &r->scatPdf, flagsNS, &stype, &draw, lamL) || !(r->scatPdf > 0)) return false;
    const bool sampledSpecular = (stype & BSDF_SPECULAR) != 0;
    const float lp = sampledSpecular ? 0.f : ((PBR_DIAG_SHADE & 4) ? 0.5f : pdf_li<NRM>(S, light, isect, wi));
    if (!(sampledSpecular || lp != 0)) return false;
    r->fB = bsdf_sample_sum<LOBES>(bsdf, isect.wo, wi, flagsNS, draw) * absdot(wi, isect.sn);
    if (black(r->fB)) return false;
    if (!sampledSpecular) {
        float fp = 1 * r->scatPdf, gp = 1 * lp;
        r->weightB = (fp * fp) / (fp * fp + gp * gp);
    }
    *probe = spawn_ray(isect, wi);
    return true;
}

// The estimate's record (beta at the estimate: the path's beta before its BSDF sample) at the
// direct queue's next position, which it returns.  Every lane of the wave calls the pushes.
__device__ __forceinline__ int push_direct(const WfpParams& X, int* counter, int base, const DirectRec& r, rgb beta) {
    const int di = base + wave_push(counter, r.pending());
    if (r.pending()) {
        X.dA[di] = make_float4(r.a.r, r.a.g, r.a.b, r.pmf);
        X.dB[di] = make_float4(r.fB.r, r.fB.g, r.fB.b, r.weightB);
        X.dBeta[di] = make_float4(beta.r, beta.g, beta.b, r.scatPdf);
        X.dFlags[di] = r.flags;
        X.dLight[di] = r.light;
    }
    return di;
}

__device__ __forceinline__ void push_probe(const WfpParams& X, int* counter, int base, bool push, const Ray& probe, int di) {
    const int pi = base + wave_push(counter, push);
    if (push) {
        X.po[pi] = make_float4(probe.o.x, probe.o.y, probe.o.z, probe.tMax);
        X.pd[pi] = make_float4(probe.d.x, probe.d.y, probe.d.z, 0.f);
        X.pid[pi] = di;
    }
}

// The path's own BSDF sample (PathIntegrator.cpp:80-105): wo is -ray.d here, not the normalised
// isect.wo the light estimate uses.  Updates beta, etaScale and specularBounce; false: the path ends.
template <int LOBES, int SMP>
__device__ __forceinline__ bool sample_bounce(const KParams& P, const BSDF& bsdf, const Isect& isect, PathEntry* e, Ray* cont) {
    const f3 wo = -e->ray.d;
    f3 wi = mk(0, 0, 0);
    float pdf = 0;
    int flags = 0;
    float u0, u1;
    get2d<true, SMP>(P.smp, e->st, &u0, &u1);
    rgb f = bsdf_sample<LOBES>(bsdf, wo, &wi, u0, u1, &pdf, BSDF_ALL, &flags);
    if (black(f) || pdf == 0.f) return false;
    e->beta = e->beta * (f * absdot(wi, isect.sn) / pdf);
    e->specularBounce = (flags & BSDF_SPECULAR) != 0;
    if ((flags & BSDF_SPECULAR) && (flags & BSDF_TRANSMISSION)) {
        float eta = bsdf.mt->eta;
        e->etaScale *= (dot(wo, isect.n) > 0) ? (eta * eta) : 1 / (eta * eta);
    }
    *cont = spawn_ray(isect, wi);
    return true;
}

// Russian roulette on the continuation (PathIntegrator.cpp:99-104); false: the path ends
template <int SMP>
__device__ __forceinline__ bool survives_roulette(const KParams& P, PathEntry* e) {
    const rgb rrBeta = e->beta * e->etaScale;
    if (maxval(rrBeta) < P.rrThreshold && e->bounces > 3) {
        float qq = mx((float).05, 1 - maxval(rrBeta));
        if (get1d<true, SMP>(P.smp, e->st) < qq) return false;
        e->beta = e->beta / (1 - qq);
    }
    return true;
}

// The end of an entry's bounce: a path that ends leaves its L in stL, one that goes on is pushed
// with its state (medium: the continuation's, -1 for Path), and the bounce's estimate learns where
// the path's L is when it resolves.  shaded: this launch finished the entry's bounce.
__device__ __forceinline__ void push_next(const WfpParams& X, int* counter, int base, bool shaded, bool pushNext, const PathEntry& e,
                                          const Ray& cont, int medium, bool pushDirect, int di) {
    const WfParams& W = X.W;
    if (shaded) {
        if (X.lastLevel) pushNext = false;   // never taken: no bounce is left at the last level
        if (!pushNext) X.stL[e.id] = make_float4(e.L.r, e.L.g, e.L.b, 0.f);
    }
    const int ni = base + wave_push(counter, pushNext);
    if (pushNext) {
        W.next.o[ni] = make_float4(cont.o.x, cont.o.y, cont.o.z, cont.tMax);
        W.next.d[ni] = make_float4(cont.d.x, cont.d.y, cont.d.z, __int_as_float(pack_path(e.st.dim, e.bounces, e.specularBounce, medium)));
        W.next.id[ni] = e.id;
        W.next.s0[ni] = make_float4(e.L.r, e.L.g, e.L.b, e.beta.r);
        W.next.s1[ni] = make_float4(e.beta.g, e.beta.b, e.etaScale, __uint_as_float(e.st.index));
    }
    if (pushDirect) X.dTgt[di] = pushNext ? ni : ~e.id;
}

// A shade launch's walk over its workgroup's queue entries, for both integrators.  The segment push
// counters s_push[4] — [0] shadow rays or transmittance walks (seg0), [1] probe rays, [2] direct
// records, [3] continuations — start at 0, or where the pass before left them, and are written back
// at the end.  shade(active, q, deferred) shades queue position q and returns the pass it leaves
// the entry to (DEFERS; 0: none); every lane of the workgroup calls it together (wave_push needs
// convergent lanes).  classify(q) is the entry's pass.
//   !CLASSED   every entry, 256 at a time;
//   pass > 0   the list pass 0 filed for this pass, dense, 256 at a time;
//   pass 0     walks every entry, files the other passes' positions in their lists and gathers its
//              own into an LDS ring: appended per iteration (at most 256), shaded 256 at a time
//              once that many are pending, so fewer than 256 wait and 512 slots never overrun.
constexpr int kDeferred = (int)0x80000000;   // pass-list entry: pass 0 began its bounce (k_wfv_shade)
template <bool CLASSED, bool DEFERS, class Classify, class Shade>
__device__ __forceinline__ void shade_entries(const WfpParams& X, int* seg0, int* s_push, int level0, int pass,
                                              const Classify& classify, const Shade& shade) {
    const WfParams& W = X.W;
    const int b = wf_block();
    if (threadIdx.x < 4) {
        int v = 0;
        if (CLASSED && pass > 0) v = threadIdx.x == 0 ? seg0[b] : threadIdx.x == 1 ? X.probeSeg[b] : threadIdx.x == 2 ? X.directSeg[b] : W.next.segCount[b];
        s_push[threadIdx.x] = v;
    }
    __syncthreads();
    const int n = level0 ? W.nSamples : seg_scan(W.cur.segCount);
    const int stride = gridDim.x * blockDim.x;
    const int nIter = (n + stride - 1) / stride;
    const int base = b * W.segCap;
    if constexpr (!CLASSED) {
        for (int it = 0; it < nIter; ++it) {   // uniform trip count
            const int i = it * stride + b * blockDim.x + threadIdx.x;
            const bool active = i < n;
            const int q = level0 ? i : seg_pos_dense(W.segCap, i, n);
            shade(active, active ? q : 0, false);
        }
    } else if (pass > 0) {
        const int cnt = X.passCnt[(pass - 1) * kWfBlocks + b];
        const int* list = X.passList + (size_t)(pass - 1) * X.passStride + base;
        for (int k0 = 0; k0 < cnt; k0 += 256) {   // uniform trip count
            const int k = k0 + (int)threadIdx.x;
            const bool active = k < cnt;
            const int e = active ? list[k] : 0;
            shade(active, e & ~kDeferred, (e & kDeferred) != 0);
        }
    } else {
        __shared__ int s_ring[512];
        __shared__ int s_tail;
        __shared__ int s_list[8];   // entries filed per later pass
        if (threadIdx.x == 0) s_tail = 0;
        if (threadIdx.x < 8) s_list[threadIdx.x] = 0;
        __syncthreads();
        // file queue position q (with its flag) in the list of pass cls (per segment, dense)
        auto file = [&](const int cls, const int q) {
            for (int c = 1; c < X.nPasses; ++c) {
                const int at = wave_push(&s_list[c - 1], cls == c);
                if (cls == c) X.passList[(size_t)(c - 1) * X.passStride + base + at] = q;
            }
        };
        auto shade_mine = [&](const bool active, const int q) {
            const int to = shade(active, q, false);
            if constexpr (DEFERS) file(to, q | kDeferred);
        };
        int head = 0;   // workgroup-uniform
        for (int it = 0; it < nIter; ++it) {
            const int i = it * stride + b * blockDim.x + threadIdx.x;
            const int qd = level0 ? i : seg_pos_dense(W.segCap, i, n);
            const int q = i < n ? qd : 0;
            const int cls = i < n ? classify(q) : -1;
            file(cls, q);
            const int at = wave_push(&s_tail, cls == 0);
            if (cls == 0) s_ring[at & 511] = q;
            __syncthreads();
            const bool full = s_tail - head >= 256;   // (the same for every lane: no append until the barrier below)
            const int qq = full ? s_ring[(head + threadIdx.x) & 511] : 0;
            __syncthreads();   // the counter and the entries are read before any wave appends again
            if (full) {
                shade_mine(true, qq);
                head += 256;
            }
        }
        __syncthreads();
        const int tail = s_tail;
        if (head < tail) {
            const bool active = head + (int)threadIdx.x < tail;
            shade_mine(active, active ? s_ring[(head + threadIdx.x) & 511] : 0);
        }
        if constexpr (DEFERS) __syncthreads();   // every wave's deferred entries are filed
        if ((int)threadIdx.x + 1 < X.nPasses) X.passCnt[threadIdx.x * kWfBlocks + b] = s_list[threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        seg0[b] = s_push[0];
        X.probeSeg[b] = s_push[1];
        X.directSeg[b] = s_push[2];
        W.next.segCount[b] = s_push[3];
    }
}

// One bounce of PathIntegrator::Li for every queued ray.
// Waves per SIMD: 3 for either lobe set (all lobes, C4: 2 → 9.58 s, 3 → 8.86 s, 4 → 9.32 s)
#ifndef PBR_WFP_OCC
#define PBR_WFP_OCC 3
#endif
// the Lambert + mirror kernel on Sobol frames (C3) and the classed shade's Lambert pass
#ifndef PBR_WFP_OCC_MM
#define PBR_WFP_OCC_MM PBR_WFP_OCC
#endif
#ifndef PBR_WFP_OCC_L
#define PBR_WFP_OCC_L PBR_WFP_OCC
#endif
// SMP: the frame's sampler type when the launch knows it (the other samplers' code — and the kernel
// parameters it reads, which otherwise spill from SGPRs into VGPR lanes — is compiled out), else -1.
// CLASSED: one of several launches per bounce, each shading the hits of the materials whose lobe set
// it is compiled for (X.matPass, pass `pass`; the passes' walks: shade_entries).  So every wave runs
// one material class with that class's registers, and only pass 0 reads every entry's hit to
// classify it.  Entries land in the queues in another order, which nothing depends on (records are
// indexed by sample or by queue position, and every L update keeps its order: this file's header).
template <bool NRM, int LOBES, bool MATS_LDS, int OCC = PBR_WFP_OCC, int SMP = -1, bool CLASSED = false>
__global__ __launch_bounds__(256, OCC) void k_wfp_shade(WfpParams X, int level0, int pass) {
    WfParams& W = X.W;
    const KParams& P = W.P;
    const DeviceScene& S = P.S;
    stage_halton_lds(P.smp);
    const MatTemplate* mats = stage_mats<MATS_LDS>(S);
    __shared__ int s_push[4];   // shadow, probe, direct, next (shade_entries)
    const int base = wf_block() * W.segCap;
    // One queued ray.  (As a lambda the body's registers are allocated apart from the loops' of
    // shade_entries: 149 → 115 VGPRs for C3, profiles/r5_classed_shade_ab.log.)
    auto shade = [&](const bool active, const int q, bool) -> int {
        // Two phases around the light-estimate pushes: the estimate's record, shadow and probe rays
        // are written as soon as they exist, so their registers are free during the path's BSDF
        // sample; only the record's target (the continuation's position) is written at the end.
        bool pushNext = false;
        bool cont2 = false;   // phase 2 runs: the path samples its BSDF
        PathEntry e;
        Ray cont;
        Isect isect;
        BSDF bsdf;
        MatTemplate texLocal;   // a textured material's per-hit lobes (make_bsdf)
        bool pushDirect;
        int di;
        {
            bool pushShadow = false, pushProbe = false;
            Ray shadow, probe;
            DirectRec rec;
            if (active) {
                load_entry(W, q, level0, level0, &e);
                const bool found = e.hit.slot >= 0;
                if (found) {
                    hit_isect<NRM>(S, e.hit, e.ray, &isect);
                    isect.medIn = isect.medOut = -1;
                }
                add_emission(S, isect, &e);
                bool alive = found && e.bounces < P.maxDepth;
                if (alive && !make_bsdf<(LOBES & kTexturedLobes) != 0>(S, mats, isect, true, &bsdf, &texLocal)) {
                    cont = spawn_ray(isect, e.ray.d);   // isect.SpawnRay(ray.d); bounces-- then ++: same bounce
                    pushNext = true;
                    alive = false;
                } else if (alive) {
                    cont2 = true;
                    const f3 wo = isect.wo;
                    if (num_components(bsdf, BSDF_ALL & ~BSDF_SPECULAR) > 0 && S.nLights > 0) {
                        // UniformSampleOneLight: light choice, then EstimateDirect's two strategies
                        const int li = sample_light(S, get1d<true, SMP>(P.smp, e.st), &rec.pmf);
                        if (rec.pmf != 0) {
                            float uL0, uL1, uS0, uS1;
                            get2d<true, SMP>(P.smp, e.st, &uL0, &uL1);
                            get2d<true, SMP>(P.smp, e.st, &uS0, &uS1);
                            const DLight& light = S.lights[li];
                            const bool delta = light.type == LT_POINT;
                            const int flagsNS = BSDF_ALL & ~BSDF_SPECULAR;
                            f3 wi = mk(0, 0, 0);
                            float lightPdf = 0;
                            VisPt vis;
                            // Lambda(wo) of the microfacet lobes, once for the estimate's two strategies
                            const float lamL = mf_lambda<LOBES>(bsdf, bsdf.to_local(wo));
                            // the light sample: its whole term, weight folded in, waits for the shadow ray
                            rgb Li = sample_li<NRM>(S, light, isect, uL0, uL1, &wi, &lightPdf, &vis);
                            rec.a = sp(0.f);
                            if (lightPdf > 0 && !black(Li)) {
                                rgb f;
                                if constexpr (PBR_DIAG_SHADE & 1) { f = sp(0.25f); rec.scatPdf = 0.5f; }
                                else f = bsdf_f_pdf<LOBES>(bsdf, wo, wi, flagsNS, &rec.scatPdf, lamL) * absdot(wi, isect.sn);
                                if (!black(f)) {
                                    if (delta) rec.a = f * Li / lightPdf;
                                    else {
                                        float fp = 1 * lightPdf, gp = 1 * rec.scatPdf;
                                        float weight = (fp * fp) / (fp * fp + gp * gp);
                                        rec.a = f * Li * weight / lightPdf;
                                    }
                                    shadow = spawn_ray_to(isect, vis.p, vis.pError, vis.n);
                                    pushShadow = true;
                                    rec.flags |= kWfpAPending;
                                }
                            }
                            rec.fB = sp(0.f);
                            if (!delta && estimate_bsdf_sample<LOBES, NRM>(S, light, bsdf, isect, uS0, uS1, lamL, &rec, &probe)) {
                                pushProbe = true;
                                rec.flags |= kWfpBPending;
                            }
                            rec.light = li;
                        }
                    }
                }
            }
            pushDirect = rec.pending();
            di = push_direct(X, &s_push[2], base, rec, e.beta);
            const int si = base + wave_push(&s_push[0], pushShadow);
            if (pushShadow) {
                W.so[si] = make_float4(shadow.o.x, shadow.o.y, shadow.o.z, shadow.tMax);
                W.sd[si] = make_float4(shadow.d.x, shadow.d.y, shadow.d.z, 0.f);
                W.sid[si] = di;
            }
            push_probe(X, &s_push[1], base, pushProbe, probe, di);
        }
        if (cont2 && sample_bounce<LOBES, SMP>(P, bsdf, isect, &e, &cont) && survives_roulette<SMP>(P, &e)) {
            pushNext = true;
            e.bounces += 1;
        }
        push_next(X, &s_push[3], base, active, pushNext, e, cont, -1, pushDirect, di);
        return 0;
    };
    shade_entries<CLASSED, false>(X, W.shadowSeg, s_push, level0, pass, [&](int q) { return entry_pass(X, q); }, shade);
}

// VisibilityTester::Unoccluded for the light-sample rays
template <int SHORT>
__global__ __launch_bounds__(256, PBR_REFILL_OCC_ANY) void k_wfp_shadow(WfpParams X) {
    WfParams& W = X.W;
    const int n = seg_scan(W.shadowSeg);
    if constexpr (kRefill > 0 && SHORT > 0 && kQuadTraversal) {
        unsigned visible = 0;   // profile field 1, added once per wave at the end
        traverse_stream<true, kAnyShort>(
            W.P.S, n, W.segCap,
            [&](int q, int* key) {
                *key = q;
                const float4 o = W.so[q], d = W.sd[q];
                return mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, -1);
            },
            [&](int q, bool hit, const Ray&, const HitRec&) {
                if (!hit) {
                    ++visible;
                    X.dFlags[W.sid[q]] |= kWfpVisible;   // the only writer of this record in this launch
                }
            },
            W.prof, KP_WFP_SHADOW);
        if (W.prof) prof_add(W.prof + KP_WFP_SHADOW * kProfFields + 1, visible);
        return;
    }
    for (int i0 = wf_block() * blockDim.x + ((int)threadIdx.x & ~63); i0 < n; i0 += gridDim.x * blockDim.x) {   // per wave
        const int i = i0 + (int)__lane_id();
        const int q = seg_pos_dense(W.segCap, i, n);
        if (i >= n) continue;
        float4 o = W.so[q], d = W.sd[q];
        Ray r = mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, -1);
        HitRec h;
        Counters c;
        const bool visible = !traverse<true, false, SHORT>(W.P.S, r, &h, &c);
        trav_diag(W.prof, KP_WFP_SHADOW, h);
        if (W.prof) prof_count(W.prof + KP_WFP_SHADOW * kProfFields + 1, visible);
        if (visible) X.dFlags[W.sid[q]] |= kWfpVisible;   // the only writer of this record in this launch
    }
}

// What probe ray q found: Li = the estimate's light's emission if that is what it hit (si.Le),
// light.Le(ray) if it escaped (Light::Le, F4 for non-infinite lights).
__device__ __forceinline__ void probe_result(const WfpParams& X, int q, bool hit, const Ray& ray, const HitRec& h) {
    const DeviceScene& S = X.W.P.S;
    const int di = X.pid[q];
    const int li = X.dLight[di];
    rgb Li = sp(0.f);
    if (hit) {
        if (S.primInfo[h.slot].z == li) {
            Isect lightIsect;
            hit_isect(S, h, ray, &lightIsect);
            Li = si_Le(S, lightIsect, -ray.d);
        }
    } else {
        Li = light_Le(S, S.lights[li], ray);
    }
    X.dLi[di] = make_float4(Li.r, Li.g, Li.b, 0.f);
}

// EstimateDirect's BSDF-sampled ray: closest hit
template <int SHORT>
__global__ __launch_bounds__(256, PBR_REFILL_OCC) void k_wfp_probe(WfpParams X) {
    WfParams& W = X.W;
    const DeviceScene& S = W.P.S;
    const int n = seg_scan(X.probeSeg);
    if constexpr (kRefill > 0 && SHORT > 0 && kQuadTraversal) {
        traverse_stream<false, kRefillShort>(
            S, n, W.segCap,
            [&](int q, int* key) {
                *key = q;
                const float4 o = X.po[q], d = X.pd[q];
                return mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, -1);
            },
            [&](int q, bool hit, const Ray& ray, const HitRec& h) { probe_result(X, q, hit, ray, h); },
            W.prof, KP_WFP_PROBE);
        return;
    }
    for (int i0 = wf_block() * blockDim.x + ((int)threadIdx.x & ~63); i0 < n; i0 += gridDim.x * blockDim.x) {   // per wave
        const int i = i0 + (int)__lane_id();
        const int q = seg_pos_dense(W.segCap, i, n);
        if (i >= n) continue;
        float4 o = X.po[q], d = X.pd[q];
        Ray ray = mkray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, -1);
        HitRec h;
        Counters c;
        const bool hit = traverse<false, false, SHORT>(S, ray, &h, &c);
        trav_diag(W.prof, KP_WFP_PROBE, h);
        probe_result(X, q, hit, ray, h);
    }
}

// the path's L where the estimate resolves: its continuation entry, or stL[id] if the path ended
__device__ __forceinline__ void add_direct(const WfpParams& X, int tgt, rgb direct) {
    float4* p = tgt >= 0 ? &X.W.next.s0[tgt] : &X.stL[~tgt];
    float4 L = *p;
    L.x = L.x + direct.r; L.y = L.y + direct.g; L.z = L.z + direct.b;
    *p = L;
}

// Ld = [A if the light sample is unoccluded] + [f·Li·weight/scatteringPdf if Li is not black];
// L += beta · (Ld / pmf) — UniformSampleOneLight's division, then PathIntegrator's beta product.
__global__ __launch_bounds__(256) void k_wfp_resolve(WfpParams X) {
    WfParams& W = X.W;
    const int n = seg_scan(X.directSeg);
    for (int i0 = wf_block() * blockDim.x + ((int)threadIdx.x & ~63); i0 < n; i0 += gridDim.x * blockDim.x) {   // per wave
        const int i = i0 + (int)__lane_id();
        const int di = seg_pos_dense(W.segCap, i, n);
        if (i >= n) continue;
        const int fl = X.dFlags[di];
        const float4 a = X.dA[di], bt = X.dBeta[di];
        rgb Ld = sp(0.f);
        if ((fl & kWfpAPending) && (fl & kWfpVisible)) Ld = Ld + sp3(a.x, a.y, a.z);
        if (fl & kWfpBPending) {
            const float4 li = X.dLi[di], b = X.dB[di];
            const rgb Li2 = sp3(li.x, li.y, li.z);
            if (!black(Li2)) Ld = Ld + sp3(b.x, b.y, b.z) * Li2 * b.w / bt.w;
        }
        const rgb beta = sp3(bt.x, bt.y, bt.z);
        add_direct(X, X.dTgt[di], beta * (Ld / a.w));
    }
}

// Per-pixel in-order sum of the per-sample L (colObj += Li) and the film; layout as k_wf_finish.
template <bool PASS>
__device__ __forceinline__ void wfp_finish(WfpParams& X) {
    WfParams& W = X.W;
    __shared__ float lds[3 * (kFinishSamples + 64)];
    __shared__ float sum[64 * 3 * (PASS ? 2 : 1)];
    const KParams& P = W.P;
    const int spp = P.spp, pitch = min(spp, kFinishSamples) + 1;
    const int pb = finish_pixels(spp);
    const int lp0 = blockIdx.x * pb;   // dispatch order: the XCD-run order made finish 28% slower
    const int npx = min(pb, W.chunkPix - lp0);
    const int slice = min(spp, kFinishSamples);
    float acc = 0.f, acc2 = 0.f;
    if constexpr (PASS) {
        if ((int)threadIdx.x < 3 * npx) {
            const long long q = W.chunkPix0 + lp0 + threadIdx.x / 3;
            acc = pass_load(P, q, threadIdx.x % 3);
            acc2 = pass_load(P, q, 3 + threadIdx.x % 3);
        }
    }
    for (int s0 = 0; s0 < spp; s0 += slice) {
        const int ns = npx * min(slice, spp - s0);
        for (int t = threadIdx.x; t < ns; t += blockDim.x) {
            const int p = spp <= kFinishSamples ? t / spp : 0, k = spp <= kFinishSamples ? t - p * spp : s0 + t;
            const float4 L = X.stL[(lp0 + p) * spp + k];
            const int kk = k - s0;
            lds[(p * 3 + 0) * pitch + kk] = L.x;
            lds[(p * 3 + 1) * pitch + kk] = L.y;
            lds[(p * 3 + 2) * pitch + kk] = L.z;
        }
        __syncthreads();
        if ((int)threadIdx.x < 3 * npx) {
            const int cnt = min(slice, spp - s0);
            const float* row = lds + threadIdx.x * pitch;
            for (int k = 0; k < cnt; ++k) {
                acc = acc + row[k];
                if constexpr (PASS) acc2 = acc2 + row[k] * row[k];
            }
        }
        __syncthreads();
    }
    finish_film<PASS>(P, W.chunkPix0 + lp0, npx, sum, acc, acc2);
}
__global__ __launch_bounds__(256) void k_wfp_finish(WfpParams X) { wfp_finish<false>(X); }
__global__ __launch_bounds__(256) void k_wfp_finish_pass(WfpParams X) { wfp_finish<true>(X); }
