// pbr_adaptive.h — adaptive sampling over the pass accumulator: the per-pixel stopping
// rule, the ordered compaction of the pixels still active into a list, and what turns such a list
// into a pass the unchanged PASS kernels render — runs of listed pixels as device-resident tiles, a
// dense working accumulator gathered from the frame's and scattered back.  Included by
// pbr_kernels.hip after the wavefront headers; no render kernel is touched.
#pragma once

constexpr int kAdaptBS = 256;
constexpr int kAdaptWave = 64;

// Rank of a flagged thread among the block's flagged threads, in thread order, and their number:
// wave ballot, then the wave counts summed over LDS.  Every thread of the block calls it.
__device__ __forceinline__ int adapt_block_rank(bool flag, int* total) {
    constexpr int NW = kAdaptBS / kAdaptWave;
    __shared__ int wcnt[NW];
    const int lane = threadIdx.x & (kAdaptWave - 1), w = threadIdx.x / kAdaptWave;
    const unsigned long long m = __ballot(flag), below = (1ull << lane) - 1ull;
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < NW; ++i) {
        if (i < w) off += wcnt[i];
        tot += wcnt[i];
    }
    __syncthreads();
    *total = tot;
    return off + __popcll(m & below);
}

// The stopping rule, float32 throughout and in this order (the build has -ffp-contract=off): with n
// samples done, the variance of the pixel mean summed over the channels, E, against the square of
// tolerance × max(mean summed over the channels, floor).  No square root, no transcendental: a float32
// restatement on the host decides exactly as this does.  A NaN anywhere: not active.
__device__ __forceinline__ bool adapt_active(const float* a, int k, float tolerance, float floor, float* Eout) {
    const float n = (float)k;
    float m[3], v[3];
    for (int c = 0; c < 3; ++c) {
        m[c] = a[c] / n;
        const float d = a[3 + c] - a[c] * m[c];
        v[c] = d > 0.f ? d : 0.f;
    }
    const float E = ((v[0] + v[1]) + v[2]) / (n * (n - 1.f));
    const float M = (m[0] + m[1]) + m[2];
    const float B = M > floor ? M : floor;
    const float T = tolerance * B;
    *Eout = E;
    return E > T * T;
}

// Entry i of the previous list (listIn == nullptr: pixel i) is considered: its E goes to errOut (if
// given), its decision to flags[i], and the block's number of active entries to blockCnt.  An entry
// outside [0, nPixels) is not considered.
__global__ __launch_bounds__(kAdaptBS) void k_adapt_select(const float* __restrict__ accum, const int32_t* __restrict__ listIn,
                                                          int n, int nPixels, int k, float tolerance, float floor,
                                                          uint8_t* __restrict__ flags, int* __restrict__ blockCnt,
                                                          float* __restrict__ errOut) {
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    bool act = false;
    if (i < n) {
        const int p = listIn ? listIn[i] : (int)i;
        if (p >= 0 && p < nPixels) {
            float a[6];
            for (int c = 0; c < 6; ++c) a[c] = accum[6 * (size_t)p + c];
            float E;
            act = adapt_active(a, k, tolerance, floor, &E);
            if (errOut) errOut[p] = E;
        }
        flags[i] = act ? 1 : 0;
    }
    int tot;
    adapt_block_rank(act, &tot);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = tot;
}

// Exclusive scan of the block counts in place, one workgroup walking them 256 at a time with a
// carry; the sum goes to *total.  nDev (if given): the element count the blocks cover, on the device.
__global__ __launch_bounds__(kAdaptBS) void k_adapt_scan(int* __restrict__ cnt, int nBlocks, const int* __restrict__ nDev,
                                                        int* __restrict__ total) {
    __shared__ int s[kAdaptBS];
    const int tid = threadIdx.x;
    if (nDev) nBlocks = (int)(((long long)*nDev + kAdaptBS - 1) / kAdaptBS);
    int carry = 0;
    for (int base = 0; base < nBlocks; base += kAdaptBS) {
        const int i = base + tid;
        const int v = i < nBlocks ? cnt[i] : 0;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < kAdaptBS; off <<= 1) {
            const int t = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        const int incl = s[tid], tot = s[kAdaptBS - 1];
        if (i < nBlocks) cnt[i] = carry + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// The flagged entries, in order, into the next list (ascending, as the previous one was).
__global__ __launch_bounds__(kAdaptBS) void k_adapt_compact(const int32_t* __restrict__ listIn, int n,
                                                           const uint8_t* __restrict__ flags, const int* __restrict__ blockOff,
                                                           int32_t* __restrict__ listOut) {
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    const bool act = i < n && flags[i] != 0;
    int tot;
    const int r = adapt_block_rank(act, &tot);
    if (act) listOut[blockOff[blockIdx.x] + r] = listIn ? listIn[i] : (int32_t)i;
}

// ---- a list as tiles.  A run: the maximal stretch of listed pixels consecutive in the frame's packed
// order within one row of one frame tile; it becomes a tile one pixel high, whose start in the dense
// (listed) order is the list position of its first pixel — pixel_xy's search over them then gives a
// dense pixel its raster position.
struct AdaptFrame {
    const int4* tiles;            // the frame's tiles and their packed starts (KParams::tiles, tileStart)
    const long long* tileStart;
    int nTiles;
    long long nPixels;
};
__device__ __forceinline__ void adapt_locate(const AdaptFrame& F, long long p, int* x, int* y, int* col) {
    int lo = 0, hi = F.nTiles - 1;
    while (lo < hi) {   // last tile with start <= p (pixel_xy)
        const int mid = (lo + hi + 1) >> 1;
        if (F.tileStart[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int4 t = F.tiles[lo];
    const long long local = p - F.tileStart[lo];
    const int w = t.z - t.x;
    *col = (int)(local % w);
    *x = t.x + *col;
    *y = t.y + (int)(local / w);
}
// n: the list's length, read from *nDev when given (an adaptive round encodes the list its select
// just wrote, before the host knows its length; the grid then covers the previous list's length).
// flags[i] = entry i starts a run.  *bad is set when the list is not ascending pixels of the frame;
// such entries are clamped, so nothing here reads or writes outside its buffers.
__global__ __launch_bounds__(kAdaptBS) void k_adapt_run_flags(const int32_t* __restrict__ list, int n, const int* __restrict__ nDev,
                                                             AdaptFrame F, uint8_t* __restrict__ flags, int* __restrict__ blockCnt,
                                                             int* __restrict__ bad) {
    if (nDev) n = *nDev;
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    bool head = false;
    if (i < n) {
        long long p = list[i];
        const long long prev = i > 0 ? (long long)list[i - 1] : -1;
        if (p < 0 || p >= F.nPixels || prev >= p) { *bad = 1; p = p < 0 ? 0 : (p >= F.nPixels ? F.nPixels - 1 : p); }
        int x, y, col;
        adapt_locate(F, p, &x, &y, &col);
        head = i == 0 || prev + 1 != p || col == 0;
        flags[i] = head ? 1 : 0;
    }
    int tot;
    adapt_block_rank(head, &tot);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = tot;
}
// A run's first entry writes its tile's corner and start, its last entry the tile's end.
__global__ __launch_bounds__(kAdaptBS) void k_adapt_run_encode(const int32_t* __restrict__ list, int n, const int* __restrict__ nDev,
                                                              AdaptFrame F, const uint8_t* __restrict__ flags,
                                                              const int* __restrict__ blockOff, int4* __restrict__ runTiles,
                                                              long long* __restrict__ runStart) {
    if (nDev) n = *nDev;
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    const bool head = i < n && flags[i] != 0;
    int tot;
    const int r = blockOff[blockIdx.x] + adapt_block_rank(head, &tot) + (head ? 1 : 0) - 1;   // the entry's run
    if (i >= n) return;
    long long p = list[i];
    p = p < 0 ? 0 : (p >= F.nPixels ? F.nPixels - 1 : p);
    int x, y, col;
    adapt_locate(F, p, &x, &y, &col);
    int* t = reinterpret_cast<int*>(runTiles + r);
    if (head) { t[0] = x; t[1] = y; runStart[r] = i; }
    if (i == n - 1 || flags[i + 1] != 0) { t[2] = x + 1; t[3] = y + 1; }
}

// The listed pixels' sums into the dense working accumulator the pass renders against ...
__global__ __launch_bounds__(kAdaptBS) void k_adapt_gather(const int32_t* __restrict__ list, int n, const float* __restrict__ accum,
                                                          float* __restrict__ dense) {
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    if (i >= n) return;
    const float* a = accum + 6 * (size_t)list[i];
    float* o = dense + 6 * (size_t)i;
    for (int c = 0; c < 6; ++c) o[c] = a[c];
}
// ... and the pass's sums and pixels back to the frame's buffers at the listed indices.
__global__ __launch_bounds__(kAdaptBS) void k_adapt_scatter(const int32_t* __restrict__ list, int n, const float* __restrict__ dAccum,
                                                           const float* __restrict__ dRgb, const uint32_t* __restrict__ dRgba,
                                                           float* __restrict__ accum, float* __restrict__ rgb,
                                                           uint32_t* __restrict__ rgba) {
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    if (i >= n) return;
    const size_t p = (size_t)list[i];
    for (int c = 0; c < 6; ++c) accum[6 * p + c] = dAccum[6 * (size_t)i + c];
    if (rgb) for (int c = 0; c < 3; ++c) rgb[3 * p + c] = dRgb[3 * (size_t)i + c];
    if (rgba) rgba[p] = dRgba[i];
}
// counts[list[i]] = value (list == nullptr: every pixel).
__global__ __launch_bounds__(kAdaptBS) void k_adapt_counts(const int32_t* __restrict__ list, int n, int32_t* __restrict__ counts,
                                                          int value) {
    const long long i = (long long)blockIdx.x * kAdaptBS + threadIdx.x;
    if (i < n) counts[list ? list[i] : i] = value;
}
