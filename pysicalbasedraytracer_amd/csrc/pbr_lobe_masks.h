// pbr_lobe_masks.h — the lobe masks the shading kernels are compiled under and the LDS copy of the
// material templates.  Included by pbr_wavefront.h (the shading kernels) and by pbr_bsdf_probe.hip
// (the BSDF probe, which evaluates one query under each of them).
#pragma once

// LOBES: the lobe kinds present in the scene (kSimpleLobes drops the microfacet code and its registers).
constexpr int kSimpleLobes = (1 << L_LAMBERT) | (1 << L_OREN) | (1 << L_SPEC_R) | (1 << L_SPEC_T) | (1 << L_FRESNEL_SPEC);
// Lambert and rough (microfacet) reflection / transmission only — matte, plastic, metal and rough
// glass: the Path/VolPath shading kernels for C4 and C5 without the specular and Oren-Nayar code
constexpr int kMicroLobes = (1 << L_LAMBERT) | (1 << L_MF_R) | (1 << L_MF_T);
// Lambert and perfect mirror reflection only — matte (σ = 0) and mirror materials: C2's dragon and
// floor, C3's scene
constexpr int kMatteMirrorLobes = (1 << L_LAMBERT) | (1 << L_SPEC_R);
// The lobe sets of the classed Path/VolPath shade (one launch per set present in the scene)
constexpr int kPassLobes[] = {1 << L_LAMBERT, 1 << L_MF_R, (1 << L_LAMBERT) | (1 << L_MF_R), (1 << L_MF_R) | (1 << L_MF_T),
                              kMicroLobes};
// MATS_LDS: the material templates fit kLdsMats and are read from an LDS copy (the BSDF code walks
// them with dependent loads).
constexpr int kLdsMats = 32;
__shared__ MatTemplate s_mats[kLdsMats];
// The templates a shade kernel reads: the scene's, or the workgroup's LDS copy of them (every thread
// calls it; the kernel's next barrier publishes the copy).
template <bool MATS_LDS>
__device__ __forceinline__ const MatTemplate* stage_mats(const DeviceScene& S) {
    if constexpr (!MATS_LDS) return S.materials;
    constexpr int words = (int)(sizeof(MatTemplate) / 4);
    const int n = 2 * S.nMaterials * words;
    const uint32_t* src = (const uint32_t*)S.materials;
    uint32_t* dst = (uint32_t*)s_mats;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    return s_mats;
}
