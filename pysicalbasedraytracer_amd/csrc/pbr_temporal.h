// pbr_temporal.h — temporal accumulation: the last frame's sums, reprojected through the
// first-hit distance and resampled bilinearly, merged into this frame's as a capped history.  Image-space
// work on two frames in raster order; no scene, queue or lane is touched, and there are no working planes.
//
// tp_pixel is the whole rule for one pixel, written once for both sides: k_tp_accumulate (below, included
// by pbr_kernels.hip after pbr_denoise.h) runs it on the device, pbr_hip_temporal_host (pbr_scene.cpp) on
// the CPU.  The rule is float32 in a fixed order, without transcendentals and (the build has
// -ffp-contract=off and correctly rounded division and square root) without fused operations, so
// tests/temporal_expected.py restates it in numpy to the bit.
//
// Two parts.  The rule (namespace pbr) is included like any header.  The kernel needs the tile constants
// of pbr_denoise.h and the film transform, which live inside pbr_kernels.hip: that file includes this one
// a second time, at that place, with PBR_TEMPORAL_KERNEL defined.
#ifndef PBR_TEMPORAL_H
#define PBR_TEMPORAL_H
#include "../../include/pbr_hip.h"
#include "pbr_math.h"

namespace pbr {

struct TpPixel {
    float s[6];     // the merged sums
    int32_t count;  // the samples behind them
    float mx, my;   // the motion: where the pixel was in the previous frame, minus where it is
};

PBR_HD bool tp_finite(float v) { return fabsf(v) <= kMaxFloat; }   // (a NaN fails the comparison)
// The demodulation divisor of a pixel from its feature image (the denoiser's rule).
PBR_HD float tp_divisor(int demodulate, const float* f, int c) {
    if (!demodulate) return 1.f;
    const float a = f[c] + (1.f - f[3]);
    return a > 0.01f ? a : 0.01f;
}

// Pixel (x, y) of the frame: steps A to D of §4.8.  The current buffers are read at the pixel's own entry
// only, and before the caller writes anything, so accum_out / counts_out may be the current buffers.
PBR_HD TpPixel tp_pixel(const pbr_temporal& T, int x, int y, int samples, const int32_t* countsCur, const float* accumCur,
                        const float* aovCur, const int32_t* countsPrev, const float* accumPrev, const float* aovPrev) {
    const int W = T.width, H = T.height;
    const size_t p = (size_t)y * W + x;
    const float* a = accumCur + 6 * p;
    const float* f = aovCur + 8 * p;
    TpPixel o;
    for (int c = 0; c < 6; ++c) o.s[c] = a[c];
    o.count = countsCur ? countsCur[p] : samples;
    o.mx = 0.f;
    o.my = 0.f;
    // A. the point the pixel's centre sees
    const float z = f[7];
    if (!(f[3] > 0.f)) return o;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float* R = T.cur_raster_to_world;
    const float X = (R[0] * fx + R[1] * fy) + R[3];
    const float Y = (R[4] * fx + R[5] * fy) + R[7];
    const float Zc = (R[8] * fx + R[9] * fy) + R[11];
    const float Wc = (R[12] * fx + R[13] * fy) + R[15];
    const float gx = X / Wc - T.cur_eye[0], gy = Y / Wc - T.cur_eye[1], gz = Zc / Wc - T.cur_eye[2];
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float Px = T.cur_eye[0] + (gx / len) * z, Py = T.cur_eye[1] + (gy / len) * z, Pz = T.cur_eye[2] + (gz / len) * z;
    // B. where the previous camera saw it
    const float* M = T.prev_world_to_raster;
    const float xp = ((M[0] * Px + M[1] * Py) + M[2] * Pz) + M[3];
    const float yp = ((M[4] * Px + M[5] * Py) + M[6] * Pz) + M[7];
    const float wp = ((M[12] * Px + M[13] * Py) + M[14] * Pz) + M[15];
    if (!(wp > 0.f)) return o;
    const float rx = xp / wp, ry = yp / wp;
    if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) return o;
    o.mx = rx - fx;
    o.my = ry - fy;
    const float ex = Px - T.prev_eye[0], ey = Py - T.prev_eye[1], ez = Pz - T.prev_eye[2];
    const float zexp = sqrtf((ex * ex + ey * ey) + ez * ez);
    // C. the four taps around it
    const float u = rx - 0.5f, v = ry - 0.5f;
    const float fx0 = floorf(u), fy0 = floorf(v);
    const float tx = u - fx0, ty = v - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;   // (-1 .. W-1, -1 .. H-1: rx and ry lie in the frame)
    const float tz = T.tol_z * zexp;
    float sw = 0.f, sm[3] = {0.f, 0.f, 0.f}, sq[3] = {0.f, 0.f, 0.f};
    int kmin = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float b = (i ? tx : 1.f - tx) * (j ? ty : 1.f - ty);
            if (!(b > 0.f)) continue;
            const size_t q = (size_t)qy * W + qx;
            const int kq = countsPrev[q];
            if (kq < 1) continue;
            const float* fq = aovPrev + 8 * q;
            if (!(fq[3] > 0.f)) continue;
            if (!(fabsf(fq[7] - zexp) <= tz)) continue;
            const float dx = f[4] - fq[4], dy = f[5] - fq[5], dz = f[6] - fq[6];
            const float en = (dx * dx + dy * dy) + dz * dz;
            if (!(en <= T.tol_n)) continue;
            const float nq = (float)kq;
            const float* aq = accumPrev + 6 * q;
            float mu[3], nu[3];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float bq = tp_divisor(T.demodulate, fq, c);
                mu[c] = (aq[c] / nq) / bq;
                nu[c] = (aq[3 + c] / nq) / (bq * bq);
                ok = ok && tp_finite(mu[c]) && tp_finite(nu[c]);
            }
            if (!ok) continue;
            sw = sw + b;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sm[c] = sm[c] + b * mu[c];
                sq[c] = sq[c] + b * nu[c];
            }
            kmin = kq < kmin ? kq : kmin;
        }
    }
    // D. the merge
    if (!(sw > 0.f)) return o;
    const int kh = kmin < T.max_history ? kmin : T.max_history;
    const float nh = (float)kh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bp = tp_divisor(T.demodulate, f, c);
        const float mh = (sm[c] / sw) * bp;
        const float qh = (sq[c] / sw) * (bp * bp);
        o.s[c] = a[c] + mh * nh;
        o.s[3 + c] = a[3 + c] + qh * nh;
    }
    o.count = o.count + kh;
    return o;
}

// What is wrong with a call's parameters (nullptr: nothing); shared by the device and the host entry.
inline const char* tp_params_error(const pbr_temporal* p, int samples, const int32_t* countsCur) {
    if (!p) return "temporal: null parameters";
    if (p->width < 1 || p->height < 1) return "temporal: width and height must be >= 1";
    if ((long long)p->width * p->height >= (1ll << 31)) return "temporal: width * height must be below 2^31";
    if (p->max_history < 1 || p->max_history > (1 << 20)) return "temporal: max_history must be 1..2^20";
    if (!(p->tol_z >= 0.f) || !(p->tol_n >= 0.f)) return "temporal: tol_z and tol_n must be >= 0";
    if (!countsCur && samples < 1) return "temporal: samples must be >= 1 (or give per-pixel counts)";
    for (int i = 0; i < 16; ++i)
        if (p->cur_raster_to_world[i] != p->cur_raster_to_world[i] || p->prev_world_to_raster[i] != p->prev_world_to_raster[i])
            return "temporal: a NaN in a matrix";
    for (int i = 0; i < 3; ++i)
        if (p->cur_eye[i] != p->cur_eye[i] || p->prev_eye[i] != p->prev_eye[i]) return "temporal: a NaN in an eye point";
    return nullptr;
}
// An output may not be one of the three history buffers (a NULL output is none of them).
inline bool tp_output_is_history(const void* out, const void* countsPrev, const void* accumPrev, const void* aovPrev) {
    return out && (out == countsPrev || out == accumPrev || out == aovPrev);
}

}  // namespace pbr
#endif   // PBR_TEMPORAL_H

#if defined(PBR_TEMPORAL_KERNEL) && !defined(PBR_TEMPORAL_KERNEL_DONE)   // (pbr_kernels.hip, behind pbr_denoise.h)
#define PBR_TEMPORAL_KERNEL_DONE
// One thread per pixel over the denoiser's 32 x 8 tiles (pbr_denoise.h), so a wave's reprojected taps
// stay close together in the previous frame.  T is wave-uniform: its matrices stay in scalar registers.
// No LDS, no atomics, no scratch.  E of §4.8 (the images) is done here.
__global__ __launch_bounds__(kDnBlock) void k_tp_accumulate(pbr_temporal T, int nbx, int samples, const int32_t* countsCur,
                                                           const float* accumCur, const float* aovCur, const int32_t* countsPrev,
                                                           const float* accumPrev, const float* aovPrev, float* accumOut,
                                                           int32_t* countsOut, float* motionOut, float* rgbOut, uint32_t* rgbaOut) {
    int x0, y0;
    dn_tile_origin(nbx, &x0, &y0);
    const int x = x0 + (int)(threadIdx.x % kDnTW), y = y0 + (int)(threadIdx.x / kDnTW);
    if (x >= T.width || y >= T.height) return;
    const pbr::TpPixel o = pbr::tp_pixel(T, x, y, samples, countsCur, accumCur, aovCur, countsPrev, accumPrev, aovPrev);
    const size_t p = (size_t)y * T.width + x;
    float* a = accumOut + 6 * p;
    for (int c = 0; c < 6; ++c) a[c] = o.s[c];
    countsOut[p] = o.count;
    if (motionOut) { motionOut[2 * p] = o.mx; motionOut[2 * p + 1] = o.my; }
    if (rgbOut || rgbaOut) {
        const float n = (float)o.count;
        const rgb col = o.count == 0 ? sp(0.f) : sp3(o.s[0] / n, o.s[1] / n, o.s[2] / n);
        if (rgbOut) { rgbOut[3 * p] = col.r; rgbOut[3 * p + 1] = col.g; rgbOut[3 * p + 2] = col.b; }
        if (rgbaOut) rgbaOut[p] = film_rgba8(col);
    }
}
#endif
