// pbr_bsdf_probe.hip — pbr_hip_bsdf, pbr_hip_phase_hg and their host twins: the scattering layer of
// pbr_device.h on caller-given directions (pbr_bsdf_probe.h), in a translation unit of its own so
// that the render kernels of pbr_kernels.hip are compiled exactly as without it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <exception>
#include <type_traits>

#include "../../include/pbr_hip.h"
#include "pbr_device.h"
#include "pbr_scene.h"
#include "pbr_probe_glue.h"

using namespace pbr;

namespace {

#include "pbr_lobe_masks.h"
#include "pbr_bsdf_probe.h"

// f(std::integral_constant<int, K>) for the lobe mask K of a pbr_bsdf_variant; false: unknown variant
template <class F>
bool with_bsdf_mask(int variant, F f) {
    switch (variant) {
    case PBR_BSDF_ALL: case PBR_BSDF_ALL_LDS: case PBR_BSDF_ALL_GLOBAL: f(std::integral_constant<int, kAllLobes>()); return true;
    case PBR_BSDF_SIMPLE: f(std::integral_constant<int, kSimpleLobes>()); return true;
    case PBR_BSDF_MATTE_MIRROR: f(std::integral_constant<int, kMatteMirrorLobes>()); return true;
    case PBR_BSDF_MICRO: f(std::integral_constant<int, kMicroLobes>()); return true;
    case PBR_BSDF_PASS_L: f(std::integral_constant<int, kPassLobes[0]>()); return true;
    case PBR_BSDF_PASS_R: f(std::integral_constant<int, kPassLobes[1]>()); return true;
    case PBR_BSDF_PASS_LR: f(std::integral_constant<int, kPassLobes[2]>()); return true;
    case PBR_BSDF_PASS_RT: f(std::integral_constant<int, kPassLobes[3]>()); return true;
    case PBR_BSDF_PASS_LRT: f(std::integral_constant<int, kPassLobes[4]>()); return true;
    case PBR_BSDF_MIRROR: f(std::integral_constant<int, 1 << L_SPEC_R>()); return true;
    case PBR_BSDF_TEXTURED: f(std::integral_constant<int, kAllLobes | kTexturedLobes>()); return true;
    default: return false;
    }
}

}  // namespace

extern "C" {

int pbr_hip_bsdf(pbr_hip_ctx* ctx, int variant, int n, const pbr_bsdf_query* queries, pbr_bsdf_record* out) {
    static_assert(sizeof(pbr_bsdf_query) == 96 && sizeof(pbr_bsdf_record) == 128, "the probe's records are packed words");
    if (!ctx || n < 0 || (n > 0 && (!queries || !out))) return PBR_E_INVALID;
    int mask = 0;
    if (!with_bsdf_mask(variant, [&](auto k) { mask = decltype(k)::value; })) return probe_fail(ctx, PBR_E_INVALID, "unknown BSDF variant");
    int lobes = 0, nTemplates = 0;
    if (int rc = probe_scene_info(ctx, &lobes, &nTemplates)) return rc;
    if (lobes & ~mask) return probe_fail(ctx, PBR_E_INVALID, "the variant's lobe mask does not cover the scene's lobe kinds");
    const bool fits = nTemplates <= kLdsMats;
    if (variant == PBR_BSDF_ALL_LDS && !fits) return probe_fail(ctx, PBR_E_INVALID, "the lobe templates do not fit the LDS copy");
    const bool lds = variant == PBR_BSDF_ALL_GLOBAL ? false : fits;
    return probe_round_trip(ctx, n, queries, (size_t)n * sizeof(pbr_bsdf_query), out, (size_t)n * sizeof(pbr_bsdf_record),
                            [&](const DeviceScene& S, hipStream_t st, const void* in, void* o) {
        const dim3 g((n + 255) / 256), b(256);
        const pbr_bsdf_query* q = (const pbr_bsdf_query*)in;
        pbr_bsdf_record* r = (pbr_bsdf_record*)o;
        with_bsdf_mask(variant, [&](auto k) {
            constexpr int K = decltype(k)::value;
            if constexpr ((K & kTexturedLobes) != 0) hipLaunchKernelGGL((k_bsdf_probe<K, false, true>), g, b, 0, st, S, n, q, r);
            else if (lds) hipLaunchKernelGGL((k_bsdf_probe<K, true, false>), g, b, 0, st, S, n, q, r);
            else hipLaunchKernelGGL((k_bsdf_probe<K, false, false>), g, b, 0, st, S, n, q, r);
        });
    });
}

int pbr_hip_bsdf_host(const pbr_material_desc* material, int variant, int n, const pbr_bsdf_query* queries, pbr_bsdf_record* out) {
    if (!material || n < 0 || (n > 0 && (!queries || !out))) return PBR_E_INVALID;
    int mask = 0;
    if (!with_bsdf_mask(variant, [&](auto k) { mask = decltype(k)::value; })) return PBR_E_INVALID;
    for (int k = 0; k < PBR_TEX_SLOTS; ++k)
        if (material->tex[k]) return PBR_E_INVALID;
    MatTemplate t[2];
    try {
        t[0] = constant_material_template(*material, false);
        t[1] = constant_material_template(*material, true);
    } catch (const std::exception&) {
        return PBR_E_INVALID;
    }
    for (const MatTemplate& m : t)
        for (int i = 0; i < m.nLobes; ++i)
            if ((1 << m.lobes[i].kind) & ~mask) return PBR_E_INVALID;
    with_bsdf_mask(variant, [&](auto k) {
        for (int i = 0; i < n; ++i) {
            const pbr_bsdf_query& q = queries[i];
            const MatTemplate* mt = q.material == 0 ? &t[q.multi_lobe ? 1 : 0] : nullptr;
            if (mt && !mt->valid) mt = nullptr;
            bsdf_probe_eval<decltype(k)::value>(mt, q, out + i);
        }
    });
    return PBR_OK;
}

// mirror_step (pbr_device.h), the step k_aov's FOLLOW instantiations take, on caller-given hits
int pbr_hip_mirror_step_host(int n, const pbr_surface_hit* hits, const float* kr, float* rays_out, int32_t* followed) {
    if (n < 0 || !hits || !kr || !rays_out || !followed) return PBR_E_INVALID;
    for (int i = 0; i < n; ++i) {
        const pbr_surface_hit& h = hits[i];
        Isect it;
        it.p = mk(h.p[0], h.p[1], h.p[2]);
        it.pError = mk(h.p_error[0], h.p_error[1], h.p_error[2]);
        it.wo = mk(h.wo[0], h.wo[1], h.wo[2]);
        it.n = mk(h.n[0], h.n[1], h.n[2]);
        it.sn = mk(h.ns[0], h.ns[1], h.ns[2]);
        it.dpdu = mk(h.dpdu[0], h.dpdu[1], h.dpdu[2]);
        it.slot = -1;
        it.medIn = h.medium_inside;
        it.medOut = h.medium_outside;
        it.u = h.uv[0];
        it.v = h.uv[1];
        Ray next = mkray(mk(0, 0, 0), mk(0, 0, 0), 0.f, -1);
        const bool ok = mirror_step(it, sp3(kr[3 * i], kr[3 * i + 1], kr[3 * i + 2]), &next);
        if (!ok) next = mkray(mk(0, 0, 0), mk(0, 0, 0), 0.f, -1);
        float* o = rays_out + (size_t)7 * i;
        o[0] = next.o.x; o[1] = next.o.y; o[2] = next.o.z;
        o[3] = next.d.x; o[4] = next.d.y; o[5] = next.d.z;
        o[6] = next.tMax;
        followed[i] = ok ? 1 : 0;
    }
    return PBR_OK;
}

int pbr_hip_phase_hg(pbr_hip_ctx* ctx, int n, const float* queries, float* out) {
    if (!ctx || n < 0 || (n > 0 && (!queries || !out))) return PBR_E_INVALID;
    return probe_round_trip(ctx, n, queries, (size_t)n * 36, out, (size_t)n * 20,
                            [&](const DeviceScene&, hipStream_t st, const void* in, void* o) {
        hipLaunchKernelGGL(k_phase_probe, dim3((n + 255) / 256), dim3(256), 0, st, n, (const float*)in, (float*)o);
    });
}

int pbr_hip_phase_hg_host(int n, const float* queries, float* out) {
    if (n < 0 || (n > 0 && (!queries || !out))) return PBR_E_INVALID;
    for (int i = 0; i < n; ++i) phase_probe_eval(queries + (size_t)9 * i, out + (size_t)5 * i);
    return PBR_OK;
}

}  // extern "C"
