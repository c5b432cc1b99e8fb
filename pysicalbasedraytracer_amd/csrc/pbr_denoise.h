// pbr_denoise.h — the edge-avoiding à-trous denoiser over the pass and feature buffers:
// prepare (sums → colour, variance and guides in the filter's domain), `iterations` wavelet levels
// ping-ponging between two colour planes, finish (remodulate, film transform).  Image-space work on a
// frame in raster order; no scene, queue or lane is touched.  Included by pbr_kernels.hip after
// pbr_aov.h.  Prepare's per-pixel arithmetic and the optional spatial variance estimate between prepare
// and level 0 are the functions of pbr_denoise_rule.h, shared with the host.
//
// The rule is float32 in a fixed order, without transcendentals and (the build has -ffp-contract=off)
// without fused operations, so tests/denoise_expected.py restates it in numpy to the bit.  Both level
// kernels run dn_filter; they differ in where a tap is read from, which changes no bit.
#pragma once

// Workgroup: kDnTW x kDnTH pixels, one thread each; a wave covers 64 / kDnTW whole rows of the tile.
#ifndef PBR_DN_TW
#define PBR_DN_TW 32
#endif
#ifndef PBR_DN_TH
#define PBR_DN_TH 8
#endif
// Levels 0 .. PBR_DN_LDS_LEVELS-1 (steps 1, 2, 4) stage the tile and its halo in LDS; the levels above
// read their taps through L2.  Tile shape and crossover as measured: DESIGN §4.5.
#ifndef PBR_DN_LDS_LEVELS
#define PBR_DN_LDS_LEVELS 3
#endif
constexpr int kDnTW = PBR_DN_TW, kDnTH = PBR_DN_TH, kDnBlock = kDnTW * kDnTH;
constexpr int kDnLdsLevels = PBR_DN_LDS_LEVELS;
static_assert(kDnBlock == 256 && kDnTW >= 8 && (kDnTW & (kDnTW - 1)) == 0, "a 256-thread tile whose width divides a wave");
static_assert(kDnLdsLevels >= 0 && kDnLdsLevels <= 3, "LDS variants exist for steps 1, 2 and 4");

// The working planes, 16 bytes per pixel each, so that a tap is two 16-byte loads:
//   xv {x_r, x_g, x_b, V}     colour and variance in the filter's domain (two planes, ping-pong)
//   nz {N_x, N_y, N_z, z}     the guides
//   gb {g, b_r, b_g, b_b}     the depth slope and the demodulation divisor, read once per pixel
//   un {u_r, u_g, u_b, n}     the per-sample second moment and the count: only for the spatial estimate
struct DnParams {
    int W, H;
    int nbx;                 // tiles per row of tiles: the grid is 1-D over nbx x nby tiles
    int step;                // 2^level
    float il, in, iz;        // 1 / sigma^2 of the three edge-stopping terms
    const float4* xvIn;
    float4* xvOut;
    const float4* nz;
    const float4* gb;
};

__device__ __forceinline__ void dn_tile_origin(int nbx, int* x0, int* y0) {
    const unsigned b = blockIdx.x;
    *x0 = (int)(b % (unsigned)nbx) * kDnTW;
    *y0 = (int)(b / (unsigned)nbx) * kDnTH;
}
// Prepare: dn_prepare_pixel (pbr_denoise_rule.h) at the thread's pixel.  U: also write the un plane the
// spatial estimate reads; a plain denoise call launches the instantiation without it.
template <bool U>
__global__ __launch_bounds__(kDnBlock) void k_dn_prepare(int W, int H, int nbx, int samples, int demodulate,
                                                        const int32_t* __restrict__ counts, const float* __restrict__ accum,
                                                        const float* __restrict__ aov, float4* __restrict__ xv,
                                                        float4* __restrict__ nz, float4* __restrict__ gb, float4* __restrict__ un) {
    int x0, y0;
    dn_tile_origin(nbx, &x0, &y0);
    const int x = x0 + (int)(threadIdx.x % kDnTW), y = y0 + (int)(threadIdx.x / kDnTW);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const DnPrepared<float4> o = dn_prepare_pixel<U, float4>(W, H, x, y, samples, demodulate, counts, accum, aov);
    xv[p] = o.xv;
    nz[p] = o.nz;
    gb[p] = o.gb;
    if (U) un[p] = o.un;
}

// One level at pixel (x, y), step s.  src.xv(qx, qy) / src.nz(qx, qy) give the previous level's planes
// at an in-frame pixel.  A tap outside the frame is skipped; a tap whose e is not below 16 (NaN
// included) is dropped: it adds to no sum.
template <class Src>
__device__ __forceinline__ float4 dn_filter(const DnParams& P, int s, int x, int y, const Src& src) {
    const int W = P.W, H = P.H;
    const float4 cp = src.xv(x, y), np = src.nz(x, y);
    const float g = P.gb[(size_t)y * W + x].x;
    const float lp = (cp.x + cp.y) + cp.z;
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float vb = 0.f;
    for (int j = -1; j <= 1; ++j) {
        const int qy = dn_clamp(y + j, H - 1);
        for (int i = -1; i <= 1; ++i) vb = vb + (k3[j + 1] * k3[i + 1]) * src.xv(dn_clamp(x + i, W - 1), qy).w;
    }
    const float D = vb + 1e-8f;
    const float zc = 1e-3f * np.w + 1e-6f;
    const float h[3] = {0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        // (unsigned: a row above the frame wraps past H; y + 2s cannot wrap)
        const unsigned qy = (unsigned)y + (unsigned)(s * j);
        if (qy >= (unsigned)H) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const unsigned qx = (unsigned)x + (unsigned)(s * i);
            if (qx >= (unsigned)W) continue;
            const int ai = i < 0 ? -i : i, aj = j < 0 ? -j : j;
            const float4 cq = src.xv((int)qx, (int)qy);
            float w = 1.f;
            if (i != 0 || j != 0) {
                const float4 nq = src.nz((int)qx, (int)qy);
                const float dl = lp - ((cq.x + cq.y) + cq.z);
                const float el = ((dl * dl) / D) * P.il;
                const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                const float en = ((dx * dx + dy * dy) + dz * dz) * P.in;
                const float dd = np.w - nq.w;
                const float den = g * (float)(s * (ai > aj ? ai : aj)) + zc;
                const float ez = ((dd * dd) / (den * den)) * P.iz;
                const float e = (el + en) + ez;
                if (!(e < 16.f)) continue;
                float t = 1.f - e * 0.0625f;
                t = t * t;
                t = t * t;
                t = t * t;
                t = t * t;
                w = t;
            }
            const float hw = (h[ai] * h[aj]) * w;
            sw = sw + hw;
            sr = sr + hw * cq.x;
            sg = sg + hw * cq.y;
            sb = sb + hw * cq.z;
            sv = sv + (hw * hw) * cq.w;
        }
    }
    return make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// The large steps: every tap through L2.
struct DnGlobalSrc {
    const float4* __restrict__ pxv;
    const float4* __restrict__ pnz;
    int W;
    __device__ __forceinline__ float4 xv(int qx, int qy) const { return pxv[(size_t)qy * W + qx]; }
    __device__ __forceinline__ float4 nz(int qx, int qy) const { return pnz[(size_t)qy * W + qx]; }
};
__global__ __launch_bounds__(kDnBlock) void k_dn_atrous(DnParams P) {
    int x0, y0;
    dn_tile_origin(P.nbx, &x0, &y0);
    const int x = x0 + (int)(threadIdx.x % kDnTW), y = y0 + (int)(threadIdx.x / kDnTW);
    if (x >= P.W || y >= P.H) return;
    const DnGlobalSrc src{P.xvIn, P.nz, P.W};
    P.xvOut[(size_t)y * P.W + x] = dn_filter(P, P.step, x, y, src);
}

// The small steps: the tile and its halo of 2 S pixels staged in LDS, both planes.  Halo pixels outside
// the frame are not loaded and never read (dn_filter skips or clamps them away).
template <int S>
struct DnLdsSrc {
    static constexpr int LW = kDnTW + 4 * S, LH = kDnTH + 4 * S;
    const float4* sxv;
    const float4* snz;
    int ox, oy;   // the frame position of LDS element (0, 0)
    __device__ __forceinline__ float4 xv(int qx, int qy) const { return sxv[(qy - oy) * LW + (qx - ox)]; }
    __device__ __forceinline__ float4 nz(int qx, int qy) const { return snz[(qy - oy) * LW + (qx - ox)]; }
};
template <int S>
__global__ __launch_bounds__(kDnBlock) void k_dn_atrous_lds(DnParams P) {
    constexpr int LW = DnLdsSrc<S>::LW, LH = DnLdsSrc<S>::LH;
    __shared__ float4 sxv[LW * LH];
    __shared__ float4 snz[LW * LH];
    int x0, y0;
    dn_tile_origin(P.nbx, &x0, &y0);
    const int ox = x0 - 2 * S, oy = y0 - 2 * S;
    for (int e = threadIdx.x; e < LW * LH; e += kDnBlock) {
        const int gx = ox + e % LW, gy = oy + e / LW;
        if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {
            const size_t q = (size_t)gy * P.W + gx;
            sxv[e] = P.xvIn[q];
            snz[e] = P.nz[q];
        }
    }
    __syncthreads();
    const int x = x0 + (int)(threadIdx.x % kDnTW), y = y0 + (int)(threadIdx.x / kDnTW);
    if (x >= P.W || y >= P.H) return;
    const DnLdsSrc<S> src{sxv, snz, ox, oy};
    P.xvOut[(size_t)y * P.W + x] = dn_filter(P, S, x, y, src);
}

// The spatial variance estimate, between prepare and level 0: dn_estimate
// (pbr_denoise_rule.h) at the thread's pixel over the tile and its halo of R pixels staged in LDS, three
// planes (xv, un, nz).  Halo pixels outside the frame are not loaded and never read.  {x, V'} goes to the
// other colour plane, so no launch reads a word it writes.  A tile none of whose pixels takes the
// estimate (every count 0 or >= minCount) copies its pixels and stages nothing.
template <int R>
struct DnSpatialSrc {
    static constexpr int LW = kDnTW + 2 * R, LH = kDnTH + 2 * R;
    const float4* sxv;
    const float4* sun;
    const float4* snz;
    int ox, oy;   // the frame position of LDS element (0, 0)
    __device__ __forceinline__ float4 xv(int qx, int qy) const { return sxv[(qy - oy) * LW + (qx - ox)]; }
    __device__ __forceinline__ float4 un(int qx, int qy) const { return sun[(qy - oy) * LW + (qx - ox)]; }
    __device__ __forceinline__ float4 nz(int qx, int qy) const { return snz[(qy - oy) * LW + (qx - ox)]; }
};
template <int R>
__global__ __launch_bounds__(kDnBlock) void k_dn_spatial(DnParams P, const float4* __restrict__ un, int minCount) {
    constexpr int LW = DnSpatialSrc<R>::LW, LH = DnSpatialSrc<R>::LH;
    __shared__ float4 sxv[LW * LH];
    __shared__ float4 sun[LW * LH];
    __shared__ float4 snz[LW * LH];
    int x0, y0;
    dn_tile_origin(P.nbx, &x0, &y0);
    const int x = x0 + (int)(threadIdx.x % kDnTW), y = y0 + (int)(threadIdx.x / kDnTW);
    const bool inside = x < P.W && y < P.H;
    const size_t p = inside ? (size_t)y * P.W + x : 0;
    float n = 0.f;
    if (inside) n = un[p].w;
    if (!__syncthreads_or(n >= 1.f && n < (float)minCount)) {
        if (inside) P.xvOut[p] = P.xvIn[p];
        return;
    }
    const int ox = x0 - R, oy = y0 - R;
    for (int e = threadIdx.x; e < LW * LH; e += kDnBlock) {
        const int gx = ox + e % LW, gy = oy + e / LW;
        if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {
            const size_t q = (size_t)gy * P.W + gx;
            sxv[e] = P.xvIn[q];
            sun[e] = un[q];
            snz[e] = P.nz[q];
        }
    }
    __syncthreads();
    if (!inside) return;
    const DnSpatialSrc<R> src{sxv, sun, snz, ox, oy};
    float4 c = src.xv(x, y);
    c.w = dn_estimate<R>(P.W, P.H, x, y, minCount, P.in, P.iz, P.gb[p].x, src);
    P.xvOut[p] = c;
}

// Finish: back out of the filter's domain, the film transform, the filtered variance.
__global__ __launch_bounds__(kDnBlock) void k_dn_finish(long long n, const float4* __restrict__ xv, const float4* __restrict__ gb,
                                                       float* __restrict__ rgbOut, uint32_t* __restrict__ rgbaOut,
                                                       float* __restrict__ varOut) {
    const long long p = (long long)blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= n) return;
    const float4 c = xv[p], b = gb[p];
    const rgb col = sp3(c.x * b.y, c.y * b.z, c.z * b.w);
    if (rgbOut) { rgbOut[3 * p] = col.r; rgbOut[3 * p + 1] = col.g; rgbOut[3 * p + 2] = col.b; }
    if (rgbaOut) rgbaOut[p] = film_rgba8(col);
    if (varOut) varOut[p] = c.w;
}
