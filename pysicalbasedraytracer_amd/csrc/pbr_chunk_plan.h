// pbr_chunk_plan.h — how the wavefront schedules cut a frame into chunks and lanes.
//
// A pure function of the schedule request, the frame's size and the memory the lanes may take: plain
// C++, no HIP types, no device state, so it compiles on any host and pbr_hip_plan_chunks
// (include/pbr_hip.h) answers without a GPU.  render_wavefront and render_wavefront_path take every
// chunking decision from wf_plan below and from nothing else.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "../../include/pbr_hip.h"
#include "pbr_config.h"

// Chunks alternate between lanes (own buffers, own stream) so one chunk's launch tails overlap
// the other's work — what keeps a small per-GPU shard of a multi-GPU frame efficient.
// Lanes a frame may use (pbr_schedule::lanes), and the default.  Measured (frame ms, bit-identical):
// C2 2 lanes 17.73-17.80, 3: 17.49, 4: 17.97 (4 lanes of 2^24-sample chunks 19.10); C3 268.7 /
// 267.3 / 274.9; C5 1396 / 1379 / 1414.
constexpr int kWfLanes = 4;
#ifndef PBR_LANES_DEFAULT
#define PBR_LANES_DEFAULT 3
#endif
constexpr int kWfDefaultLanes = PBR_LANES_DEFAULT;
// workgroups of the queue kernels = segments of a queue (pbr_wavefront.h: kWfBlocks)
#ifndef PBR_WF_BLOCKS
#define PBR_WF_BLOCKS 2048
#endif
constexpr int kWfPlanBlocks = PBR_WF_BLOCKS;

// Chunking of the wavefront schedules: at most 2^chunkLog2 samples per chunk; chunks alternate
// over the lanes.  Measured on C2: two lanes 23.4 ms vs 24.9 for one; forcing a one-chunk
// (1/8-frame shard) frame into two concurrent half chunks was slower (4.00 vs 3.86 ms).
struct WfChunks {
    long long chunkPix = 1;
    long long nChunks = 1;
    int lanes = 1;
    int chunkLog2 = 0;        // the chosen bound: at most 2^chunkLog2 samples per chunk
    size_t cap = 0;           // samples of the largest chunk
    int segCap = 0;           // capacity of one queue segment
    size_t qcap = 0;          // queue entries
    double bytesPerSample = 0;   // estimate of a lane's buffers per queue entry (an upper bound)
    double budget = 0;        // bytes the lanes may take (0: unknown)
    bool fuseCamera = false;  // Whitted: the level-0 shade traces its own camera rays
};
// A call that ran no wavefront schedule (the megakernel; no render yet): no lanes, no chunks.
inline WfChunks wf_no_chunks() {
    WfChunks c;
    c.chunkPix = c.nChunks = 0;
    c.lanes = 0;
    return c;
}
// A batch's one-chunk frames rotate over the lanes, and every lane holds queue and record buffers for
// the whole frame: they keep several lanes only while the lanes' buffers together stay within this
// many bytes (bytesPerSample × samples per lane, estimated from the schedule's buffers).  A C2 rank
// shard (≤ 2^25 samples, ≈ 12 GB per lane) keeps three; a Path frame at the 2^26-sample cap (≈ 23
// GB per lane) two; the single-frame call would run such a frame on one lane.
constexpr double kBatchLaneBytes = 48e9;
// The largest chunk a Whitted schedule accepts (its default is 2^25, less with several lights).
// Measured, C2 in 5-frame batches (bit-identical): 2^25 (four chunks) 13.62-13.69 ms, 2^26 14.39-14.61,
// 2^27 14.16-14.25 (profiles/r6_c2_chunk_ab.log).
#ifndef PBR_WF_WHITTED_MAXLOG2
#define PBR_WF_WHITTED_MAXLOG2 25
#endif
constexpr int kWfMinLog2 = 20;   // the default chunk never shrinks below 2^20 samples

// The default chunk is the largest 2^k <= 2^min(defLog2, maxLog2) samples (defLog2 0: maxLog2) whose
// lanes' buffers fit laneBudget bytes, not below 2^kWfMinLog2; with laneBudget 0 (unknown) it is that
// start itself.  A batch's one-chunk frames keep as many lanes as fit laneBudget (0: kBatchLaneBytes).
// A requested chunk_log2 is capped at maxLog2 and otherwise taken as is.
// wideLanes > the default lane count: the default lanes when that many lanes of 2^maxLog2-sample
// chunks fit laneBudget (the Path schedule: 4).
inline WfChunks wf_chunks(const pbr_schedule& sch, long long nPixels, int spp, int maxLog2, bool batch,
                          double bytesPerSample, double laneBudget, int defLog2, int wideLanes) {
    WfChunks c;
    c.bytesPerSample = bytesPerSample;
    c.budget = laneBudget;
    c.lanes = sch.serial ? 1 : (sch.lanes > 0 ? std::min(sch.lanes, kWfLanes) : kWfDefaultLanes);
    if (!sch.serial && sch.lanes == 0 && wideLanes > c.lanes && sch.chunk_log2 == 0 && laneBudget > 0 &&
        wideLanes * bytesPerSample * (double)(1LL << maxLog2) <= laneBudget)
        c.lanes = std::min(wideLanes, kWfLanes);
    int chunkLog2 = defLog2 > 0 ? std::min(defLog2, maxLog2) : maxLog2;
    if (sch.chunk_log2 > 0) chunkLog2 = std::min(sch.chunk_log2, maxLog2);
    else if (laneBudget > 0 && bytesPerSample > 0)
        while (chunkLog2 > kWfMinLog2 && c.lanes * bytesPerSample * (double)(1LL << chunkLog2) > laneBudget) --chunkLog2;
    c.chunkLog2 = chunkLog2;
    spp = std::max(1, spp);
    nPixels = std::max(1LL, nPixels);
    c.chunkPix = std::max(1LL, (1LL << chunkLog2) / spp);
    if (c.chunkPix >= nPixels) {   // one chunk: splitting a small frame only adds launch tails
        c.chunkPix = nPixels;
        if (!batch) c.lanes = 1;   // (a batch's one-chunk frames rotate over the lanes)
        else if (c.lanes > 1 && bytesPerSample > 0) {
            const double perLane = bytesPerSample * (double)nPixels * (double)spp;
            const double budget = laneBudget > 0 ? laneBudget : kBatchLaneBytes;
            c.lanes = (int)std::max(1.0, std::min((double)c.lanes, std::floor(budget / perLane)));
        }
    } else {
        // Many chunks: make them equal and a whole number per lane (the count rounded down to a
        // multiple of the lanes), so no lane runs a last chunk alone.  Measured (bit-identical,
        // frame ms; default / rounded down / rounded up): C5 (32 chunks) 1215 / 1193 / 1200, C4
        // (254) 6628 / 6587 / 6572, C3 (16) 257.0 / 257.5 / 268.3, C2 (4) 17.5 / 18.6 / 18.3 —
        // with few chunks the power-of-two size wins, so only 24 or more are balanced.
        long long n = (nPixels + c.chunkPix - 1) / c.chunkPix;
        if (n >= 24) {
            n = std::max<long long>(c.lanes, n / c.lanes * c.lanes);
            c.chunkPix = (nPixels + n - 1) / n;
            // chunks of ceil(nPixels / n) pixels can come out fewer than n when the frame has few
            // pixels per chunk (257 pixels in 32 chunks of 9 are 29): grow the chunk until the count
            // is a whole number per lane again (at the latest at one chunk per lane)
            while (((nPixels + c.chunkPix - 1) / c.chunkPix) % c.lanes != 0 && c.chunkPix < nPixels) ++c.chunkPix;
        }
    }
    c.nChunks = (nPixels + c.chunkPix - 1) / c.chunkPix;
    c.cap = (size_t)c.chunkPix * (size_t)spp;
    // a shade workgroup processes at most ceil(cap / (blocks·256)) rounds of 256
    c.segCap = (int)((c.cap + (size_t)kWfPlanBlocks * 256 - 1) / ((size_t)kWfPlanBlocks * 256) * 256);
    c.qcap = std::max(c.cap, (size_t)c.segCap * kWfPlanBlocks);
    return c;
}

// What a schedule's plan depends on besides the request (pbr_chunk_query).
struct WfPlanIn {
    int integrator = PBR_INTEGRATOR_WHITTED;
    long long nPixels = 1;
    int spp = 1;
    int maxDepth = 1;
    int nLights = 1;
    bool skyLight = false;     // the single light is a SkyBox (Whitted: its radiance is looked up by the shadow kernel)
    bool batch = false;        // pbr_hip_render_frames / pbr_hip_render_passes
    bool sceneFusable = true;  // Whitted: the scene's materials allow the fused level-0 shade
    double laneBudget = 0;     // bytes the lanes' buffers may take (lane_budget); 0: the memory query failed
};

// Whitted: records per sample and level: A, F+cos, pdf (36 B) + per light 17 B (multi-light scenes:
// per (level, light) records and up to nL shadow rays per shading event); the chunk shrinks so they
// stay under 8 GB per lane (C2: 5 levels × 36 B × 2^25 = 6 GB).
constexpr double kWhittedRecordBytes = 8e9;
inline int whitted_levels(int maxDepth) { return maxDepth < 1 ? 1 : maxDepth; }
inline bool whitted_multi_light(int nLights) { return nLights != 1; }
inline int whitted_lights_per_shade(int nLights) { return whitted_multi_light(nLights) ? std::max(1, nLights) : 1; }
inline int whitted_def_log2(int maxDepth, int nLights) {
    const int levels = whitted_levels(maxDepth);
    const bool ml = whitted_multi_light(nLights);
    int log2 = 25;
    while (log2 > kWfMinLog2 && (double)levels * (36.0 + (ml ? 17.0 * nLights : 0.0)) * (double)(1LL << log2) > kWhittedRecordBytes)
        --log2;
    return log2;
}
// Whitted's lane buffers per queue entry: two ray queues (52 B each), the shadow queue(s) — 36 B per
// entry and light, 16 more under a deferred SkyBox, and 16 B of contribution per shading event — the
// records, the sample's depth and index.  (A single frame of one chunk runs one lane with a second
// shadow queue on a stream of its own, which this does not count: one lane is never what the budget
// bounds.)
inline double whitted_bytes_per_sample(int maxDepth, int nLights, bool skyLight) {
    const int levels = whitted_levels(maxDepth);
    const bool ml = whitted_multi_light(nLights);
    const bool skyDeferred = !ml && skyLight;
    return 2 * 52.0 + (52.0 + (skyDeferred ? 16.0 : 0.0)) * whitted_lights_per_shade(nLights) + 16.0 +
           levels * (36.0 + (ml ? 17.0 * nLights : 0.0)) + 8.0;
}
// Path / VolPath: two ray queues with their state (84 B each), shadow and probe queues, the direct
// records, the sample's L and index (+ VolPath's transmittance walk and records), and the class pass
// lists (at most 5 passes of 4 B).  ≈ 19.5 GB per 2^26 chunk and lane.  Measured (bit-identical):
// C3 2^25 349.4 ms, 2^26 336.1, 2^27 340.4; C5 2^25 1979 ms, 2^26 1939, 2^27 1919.
inline double path_bytes_per_sample(bool vol) { return (vol ? 460.0 : 340.0) + 4.0 * 5; }
constexpr int kPathMaxLog2 = 27;
// Path: four lanes where four lanes of 2^27-sample chunks fit the budget (bit-identical, 2^27
// chunks, frame ms in batches: C3 204.5 → 195.8, C4 4217 → 4160; VolPath's four lanes would have to
// drop to 2^26 chunks: C5 776.6 → 806.0, profiles/r6_lanes4_batch.log)
constexpr int kPathWideLanes = 4;
// Path / VolPath when the memory query failed: 2^26-sample chunks on the default lanes (≈ 70 GB of
// lane buffers, which every MI300-class device holds) instead of an unbounded 2^27.
constexpr int kPathBlindLog2 = 26;

inline WfChunks wf_plan(const pbr_schedule& sch, const WfPlanIn& in) {
    if (in.integrator == PBR_INTEGRATOR_WHITTED) {
        WfChunks c = wf_chunks(sch, in.nPixels, in.spp, PBR_WF_WHITTED_MAXLOG2, in.batch,
                               whitted_bytes_per_sample(in.maxDepth, in.nLights, in.skyLight), in.laneBudget,
                               whitted_def_log2(in.maxDepth, in.nLights), 0);
        // The level-0 shade traces its own camera rays (no camera kernel and queue).  Frames with fewer
        // chunks than lanes (rank shards of a multi-GPU C2 job) keep the separate kernels by default:
        // there the camera kernel's 8 waves per SIMD win (C2 shard 0/8, one chunk: 2.58 → 3.10 ms fused;
        // shard 0/2, two chunks: 9.58-9.63 → 10.12-10.22).
        // Round 6: a batch whose few-chunk frames rotate over the lanes (a rank's shard) fuses as well — its
        // frames overlap on the lanes, which hides the fused kernel's lower occupancy: C2 8-rank shards
        // 2.10-2.19 → 1.99-2.02 ms, 4-rank 4.13-4.31 → 3.95-4.01 (profiles/r6_shard_c2*.json).
        const bool rotating = in.batch && c.nChunks < c.lanes;
        c.fuseCamera = in.sceneFusable && sch.fuse_camera != PBR_FUSE_OFF && !whitted_multi_light(in.nLights) &&
                       (c.nChunks >= std::max(2, c.lanes) || sch.fuse_camera == PBR_FUSE_ON || rotating);
        return c;
    }
    const bool vol = in.integrator == PBR_INTEGRATOR_VOLPATH;
    return wf_chunks(sch, in.nPixels, in.spp, kPathMaxLog2, in.batch, path_bytes_per_sample(vol), in.laneBudget,
                     in.laneBudget > 0 ? 0 : kPathBlindLog2, vol ? 0 : kPathWideLanes);
}
