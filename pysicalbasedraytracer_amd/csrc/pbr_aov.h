// pbr_aov.h — feature buffers (pbr_hip_render_aov): per pixel the albedo, coverage,
// shading normal and distance of the first surface each camera sample sees, summed over the same
// camera samples as the beauty image.  No reference counterpart; defined on the bits in pbr_hip.h.
//
// One fused kernel, no queues, no per-sample records, no chunk lanes: a workgroup holds whole pixels
// (pbr_aov_plan.h), a lane draws one sample with the render's own sampler positioning and camera
// function (sample_index, camera_sample_ray), the wave walks the BVH as a packet (traverse_wave, as
// k_wfp_camera_extend does — or each lane the binary walk, in a tree too deep for the quad walk), a
// hit without a material is passed through as the three Li's pass it (SpawnRay(ray.d), up to
// kMaxPassThrough crossings, then the device guard), and the sample's eight values go to an LDS tile
// [channel][sample slot].  One thread per (pixel, channel) then continues the carried sum over the
// pixel's slots in sample order, acc = acc + v, which is what makes any cut into passes exact (§4.2).
// A pixel of more than 256 samples is alone in its workgroup and takes several rounds, eight threads
// carrying its sums from round to round.
// (included by pbr_kernels.hip inside its unnamed namespace, after pbr_aov_plan.h at file scope)
#pragma once

constexpr int kAovChannels = PBR_AOV_CHANNELS;
constexpr int kAovMaxBounces = 16;   // pbr_hip_render_aov_mirrors' max_bounces (Whitted's kWfMaxDepth levels)
constexpr int kAovPitch = kAovBlock + 1;
static_assert(kAovChannels == 8, "a thread's (pixel, channel) is (t >> 3, t & 7)");

// KParams by value plus the kernel's own pointers (KParams keeps its size and layout).  P.spp: the
// pass's samples per pixel; P.smp.passFirst: the number of its first; P.ppb = aov_pixels_per_block.
struct AovParams {
    KParams P;
    long long pix0, pixEnd;   // this launch's packed pixels [pix0, pixEnd)
    float* accum;             // 8 floats per packed pixel of the frame: the carried sums
    float* out;               // the image (8 floats per pixel), or null
    const float4* albedo;     // per material: material_albedo of its constants, w = its pbr_material_type (0: no BSDF)
    int maxBounces;           // FOLLOW: the mirror steps a sample's chain may take (1..16)
};

// The one texture a textured material's albedo reads, through its UVMapping2D, then the material's
// clamp: textured_template's operations for that parameter alone.
__device__ __forceinline__ void aov_tex_albedo(const TexMat* texMats, const TexDev* textures, const float4* texels, int mat, float u,
                                               float v, float* a) {
    const int k = material_albedo_slot(texMats[mat].p.type);
    if (k < 0) return;
    const int ti = texMats[mat].tex[k];
    if (ti < 0) return;
    const TexDev t = textures[ti];
    const float4 val = tex_lookup(texels, t, t.su * u + t.du, t.sv * v + t.dv);
    a[0] = clampf(val.x, 0, PBR_INF); a[1] = clampf(val.y, 0, PBR_INF); a[2] = clampf(val.z, 0, PBR_INF);
}

// Waves per SIMD.  The camera kernels hold the packet walk at 8 (59 VGPRs), but this kernel also forms
// the interaction of the hit (hit_isect: sphere and triangle), and at the 64 registers of 8 waves that
// spills: compiled at each bound, untextured / textured packet-walk instantiation, VGPRs spilled →
// scratch bytes per lane: 8 waves 15 → 64 / 20 → 80, 7 waves 8 → 48 / 10 → 48, 6 waves 4 → 32 / 4 → 32,
// 5 waves 0 → 0.  Five it is (profiles/aov_resource_usage.md).  As compiled today at that bound
// (profiles/aov_follow_resource_usage.md): 91 VGPRs untextured and 95 textured, no scratch; the NRM
// instantiations (per-vertex normals, added since) 96 VGPRs with 4 spilled, 32 scratch bytes per lane.
constexpr int kAovOcc = 5;
// The FOLLOW instantiations carry seven more values across the walk (the record: albedo product, ns, T):
// at 5 waves the packet-walk ones spill 1 (untextured) to 6 VGPRs, 16-32 scratch bytes per lane, touched once
// per chain surface and not inside the walk; at 4 waves none (profiles/aov_follow_resource_usage.md).
#ifndef PBR_AOV_FOLLOW_OCC
#define PBR_AOV_FOLLOW_OCC 5
#endif
constexpr int kAovFollowOcc = PBR_AOV_FOLLOW_OCC;

// TEX: the scene has image textures (else their evaluation is compiled out, as make_bsdf<TEX>);
// BINARY: the scene runs the per-lane binary walk (DeviceScene::binaryWalk), whose stack is scratch;
// FOLLOW: mirror bounces are followed (pbr_hip_render_aov_mirrors with max_bounces > 0).
// A followed chain stays inside the walk loop, as a crossing does: at every surface with a BSDF the lane
// forms the interaction, multiplies the albedo in, and keeps (albedo product, ns, T) as its record; a
// Mirror there, below the bound, replaces the ray by mirror_step's and the lane stays pending, while
// lanes whose chains ended keep their record under the mask.  A continuation that misses leaves the
// record of the mirror it left.
template <bool NRM, bool TEX, bool BINARY, bool FOLLOW = false>
__global__ __launch_bounds__(256, FOLLOW ? kAovFollowOcc : kAovOcc) void k_aov(AovParams A) {
    __shared__ float tile[kAovChannels * kAovPitch];
    __shared__ float sums[kAovChannels * kAovBlock];
    const KParams& P = A.P;
    const DeviceScene& S = P.S;
    const int tid = threadIdx.x;
    const int spp = P.spp, first = P.smp.passFirst;
    const long long pixBase = A.pix0 + (long long)blockIdx.x * P.ppb;
    const long long rem = A.pixEnd - pixBase;
    const int npix = rem < P.ppb ? (int)rem : P.ppb;
    if (npix <= 0) return;
    const int total = npix * spp;            // sample slots, pixel-major; <= 256 unless the pixel is alone
    const bool rounds = total > kAovBlock;   // (then npix == 1: thread c < 8 carries channel c)
    const int nsum = npix * kAovChannels;
    float carry = 0.f;
    if (rounds && tid < kAovChannels && first > 0) carry = A.accum[kAovChannels * pixBase + tid];
    for (int base = 0; base < total; base += kAovBlock) {
        const int slot = base + tid;
        const bool live = slot < total;
        Ray r = mkray(mk(0, 0, 0), mk(0, 0, 1), PBR_INF, -1);
        if (live) {
            const int lp = slot / spp, sn = first + (slot - lp * spp);   // the sample's number in the pixel
            int x, y;
            pixel_xy(P, pixBase + lp, &x, &y);
            SState st;   // GlobalSampler::StartPixel/SetSampleNumber, as k_render's
            st.index = sample_index(P.smp, x, y, sn).lo;
            st.sid = sn;   // (Sobol: the index's bits >= 32 follow from the number itself)
            st.dim = 0;
            st.px = x;
            st.py = y;
            r = camera_sample_ray(P, st, x, y);
        }
        // closest hit, through material-less surfaces
        // (only the hit record lives across the walk: the interaction is formed where it is read, once for
        // a crossing and once for the recorded hit, which keeps the packet walk's 64 registers free of it)
        bool pending = live, hit = false;
        float tsum = 0.f;
        int crossings = 0, mat = -1;
        // FOLLOW: the record of the last surface with a BSDF the chain reached (recA doubles as the running product)
        float recA[3] = {0.f, 0.f, 0.f};
        f3 recNs = mk(0, 0, 0);
        float recT = 0.f;
        int steps = 0;
        bool have = false;
        HitRec h;
        h.slot = -1; h.b0 = h.b1 = h.b2 = 0.f;
        while (__builtin_amdgcn_ballot_w64(pending) != 0ull) {
            // (a lane that is done keeps its recorded hit while others go on: the walks write only live lanes')
            if (pending) { h.slot = -1; h.b0 = h.b1 = h.b2 = 0.f; }
            bool f;
            if constexpr (!BINARY && kPacket && kQuadTraversal) {
                f = traverse_wave<false>(S, r, &h, pending);
            } else {
                Counters c;
                f = pending && traverse<false, false>(S, r, &h, &c);
            }
            bool again = false;
            if (pending) {
                hit = f;
                if (f) {
                    mat = S.primInfo[h.slot].y;
                    if (mat < 0 || A.albedo[mat].w == 0.f) {   // !isect.bsdf: a medium boundary
                        if (++crossings > kMaxPassThrough) {
                            atomicOr(S.guard, kGuardWhittedPassThrough);
                            hit = false;
                            have = false;
                        } else {
                            Isect cross;
                            hit_isect<NRM>(S, h, r, &cross);
                            tsum = tsum + r.tMax;
                            r = spawn_ray(cross, r.d);
                            again = true;
                        }
                    } else if constexpr (FOLLOW) {
                        Isect si;
                        hit_isect<NRM>(S, h, r, &si);
                        const float4 a = A.albedo[mat];
                        float al[3] = {a.x, a.y, a.z};
                        if constexpr (TEX) {
                            if (S.texMats) aov_tex_albedo(S.texMats, S.textures, S.texels, mat, si.u, si.v, al);
                        }
                        if (have) { recA[0] = recA[0] * al[0]; recA[1] = recA[1] * al[1]; recA[2] = recA[2] * al[2]; }
                        else { recA[0] = al[0]; recA[1] = al[1]; recA[2] = al[2]; }
                        have = true;
                        recNs = si.sn;
                        tsum = tsum + r.tMax;
                        recT = tsum;
                        if (steps < A.maxBounces && a.w == (float)PBR_MAT_MIRROR) {
                            Ray next;
                            if (mirror_step(si, sp3(al[0], al[1], al[2]), &next)) {
                                r = next;
                                ++steps;
                                again = true;
                            }
                        }
                    }
                }
            }
            pending = again;
        }
        float alb[3] = {0.f, 0.f, 0.f};
        f3 ns = mk(0, 0, 0);
        float t = 0.f;
        if constexpr (FOLLOW) {
            hit = have;   // (a continuation that missed leaves the record of the mirror it left)
            alb[0] = recA[0]; alb[1] = recA[1]; alb[2] = recA[2];
            ns = recNs;
            t = recT;
        } else if (hit) {
            Isect si;
            hit_isect<NRM>(S, h, r, &si);
            const float4 a = A.albedo[mat];
            alb[0] = a.x; alb[1] = a.y; alb[2] = a.z;
            if constexpr (TEX) {
                if (S.texMats) aov_tex_albedo(S.texMats, S.textures, S.texels, mat, si.u, si.v, alb);
            }
            ns = si.sn;
            t = tsum + r.tMax;
        }
        tile[0 * kAovPitch + tid] = alb[0];
        tile[1 * kAovPitch + tid] = alb[1];
        tile[2 * kAovPitch + tid] = alb[2];
        tile[3 * kAovPitch + tid] = hit ? 1.f : 0.f;
        tile[4 * kAovPitch + tid] = ns.x;
        tile[5 * kAovPitch + tid] = ns.y;
        tile[6 * kAovPitch + tid] = ns.z;
        tile[7 * kAovPitch + tid] = t;
        __syncthreads();
        if (!rounds) {
            for (int k = tid; k < nsum; k += kAovBlock) {
                const int p = k >> 3, c = k & 7;
                float acc = first > 0 ? A.accum[kAovChannels * pixBase + k] : 0.f;   // (the first pass does not read accum)
                const float* row = tile + c * kAovPitch + p * spp;
                for (int s = 0; s < spp; ++s) acc = acc + row[s];
                sums[k] = acc;
            }
        } else if (tid < kAovChannels) {
            const int n = total - base < kAovBlock ? total - base : kAovBlock;
            const float* row = tile + tid * kAovPitch;
            for (int s = 0; s < n; ++s) carry = carry + row[s];
        }
        __syncthreads();
    }
    if (rounds) {
        if (tid < kAovChannels) sums[tid] = carry;
        __syncthreads();
    }
    const float done = (float)(first + spp);
    for (int k = tid; k < nsum; k += kAovBlock) {
        const float v = sums[k];
        const long long at = kAovChannels * pixBase + k;
        A.accum[at] = v;
        if (A.out) {
            const int c = k & 7;
            if (c < 7) {
                A.out[at] = v / done;
            } else {   // the mean distance of the samples that hit
                const float h = sums[k - 4];
                A.out[at] = h > 0.f ? v / h : 0.f;
            }
        }
    }
}
