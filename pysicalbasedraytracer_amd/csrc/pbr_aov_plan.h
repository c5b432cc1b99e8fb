// pbr_aov_plan.h — how a feature pass (pbr_hip_render_aov, pbr_aov.h) is cut into launches.  A pure
// host function of the pass's pixels and samples, as pbr_chunk_plan.h is for the render schedules: the
// render entry runs it, pbr_hip_plan_aov answers from it, and the CPU tests sweep it.
//
// A workgroup of 256 threads holds whole pixels (aov_pixels_per_block), and a launch's kernel numbers
// its sample slots in 32-bit words, so every launch stays below 2^31 samples and 2^31 workgroups:
// C4 (8,294,400 pixels × 1024 samples = 8.49 G) takes four launches.  Launches are consecutive ranges
// of the descriptor's packed pixel order, each but the last a whole number of workgroups.
#pragma once
#include <cstdint>
#include <vector>

namespace pbr {

constexpr int kAovBlock = 256;                       // threads of a workgroup = sample slots of a round
constexpr long long kAovMaxSamples = (1ll << 31) - 1;   // per launch

struct AovLaunch {
    long long pix0, nPix;   // packed pixels [pix0, pix0 + nPix)
};

// Pixels of one workgroup: as many whole pixels as fit one round of sample slots.
inline int aov_pixels_per_block(int samples) { return samples >= kAovBlock ? 1 : kAovBlock / samples; }

// Pixels of a full launch: the largest whole number of workgroups whose samples stay below 2^31 (its
// workgroups, at most one per pixel, then do too); at least one workgroup.
inline long long aov_launch_pixels(int samples) {
    const long long ppb = aov_pixels_per_block(samples);
    long long px = kAovMaxSamples / samples;
    px -= px % ppb;
    return px < ppb ? ppb : px;
}

inline std::vector<AovLaunch> aov_launches(long long nPixels, int samples) {
    std::vector<AovLaunch> out;
    if (nPixels < 1 || samples < 1) return out;
    const long long step = aov_launch_pixels(samples);
    for (long long p = 0; p < nPixels; p += step) out.push_back(AovLaunch{p, nPixels - p < step ? nPixels - p : step});
    return out;
}

}  // namespace pbr
