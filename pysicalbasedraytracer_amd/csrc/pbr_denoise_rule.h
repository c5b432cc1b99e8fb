// pbr_denoise_rule.h — the per-pixel arithmetic of the denoiser's prepare step and of the
// spatial variance estimate that follows it, written once for both sides: k_dn_prepare and
// k_dn_spatial (pbr_denoise.h) run these functions on the device, pbr_hip_spatial_variance_host
// (pbr_scene.cpp) on the CPU.  V4 is any {x, y, z, w} of floats: float4 on the device, DnHost4 here.
//
// The rule is float32 in a fixed order, without transcendentals and (the build has -ffp-contract=off and
// correctly rounded division) without fused operations, so tests/denoise_expected.py and
// tests/spatial_variance_expected.py restate it in numpy to the bit.
#pragma once
#include "../../include/pbr_hip.h"
#include "pbr_math.h"

namespace pbr {

struct DnHost4 { float x, y, z, w; };
template <class V4>
PBR_HD V4 dn_v4(float x, float y, float z, float w) {
    V4 v;
    v.x = x; v.y = y; v.z = z; v.w = w;
    return v;
}
PBR_HD int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
PBR_HD bool dn_finite(float v) { return fabsf(v) <= kMaxFloat; }   // (a NaN fails the comparison)

// The working planes of one pixel, 16 bytes each:
//   xv {x_r, x_g, x_b, V}     colour and variance of the pixel mean in the filter's domain
//   nz {N_x, N_y, N_z, z}     the guides
//   gb {g, b_r, b_g, b_b}     the depth slope and the demodulation divisor
//   un {u_r, u_g, u_b, n}     the per-sample second moment in the filter's domain and the count as a
//                             float (0 where the count is below 1); formed only when U
template <class V4>
struct DnPrepared { V4 xv, nz, gb, un; };

// Prepare at pixel (x, y).  k: the pixel's sample count.  Mean and variance of the mean per channel (the
// adaptive rule's arithmetic), demodulated by the first-hit albedo where a sample hit and by 1 where it
// missed.
template <bool U, class V4>
PBR_HD DnPrepared<V4> dn_prepare_pixel(int W, int H, int x, int y, int samples, int demodulate, const int32_t* counts,
                                       const float* accum, const float* aov) {
    const size_t p = (size_t)y * W + x;
    const int k = counts ? counts[p] : samples;
    const float* a = accum + 6 * p;
    const float* f = aov + 8 * p;
    float m[3], v[3], b[3];
    if (k >= 2) {
        const float n = (float)k;
        const float nn = n * (n - 1.f);
        for (int c = 0; c < 3; ++c) {
            m[c] = a[c] / n;
            const float d = a[3 + c] - a[c] * m[c];
            v[c] = (d > 0.f ? d : 0.f) / nn;
        }
    } else {
        for (int c = 0; c < 3; ++c) {
            m[c] = k == 1 ? a[c] : 0.f;
            v[c] = 0.f;
        }
    }
    for (int c = 0; c < 3; ++c) {
        if (demodulate) {
            const float al = f[c] + (1.f - f[3]);
            b[c] = al > 0.01f ? al : 0.01f;
        } else {
            b[c] = 1.f;
        }
    }
    const float V = (v[0] / (b[0] * b[0]) + v[1] / (b[1] * b[1])) + v[2] / (b[2] * b[2]);
    const int xl = dn_clamp(x - 1, W - 1), xr = dn_clamp(x + 1, W - 1), yu = dn_clamp(y - 1, H - 1), yd = dn_clamp(y + 1, H - 1);
    const float gx = fabsf(aov[8 * ((size_t)y * W + xr) + 7] - aov[8 * ((size_t)y * W + xl) + 7]);
    const float gy = fabsf(aov[8 * ((size_t)yd * W + x) + 7] - aov[8 * ((size_t)yu * W + x) + 7]);
    const float g = (gx > gy ? gx : gy) * 0.5f;
    DnPrepared<V4> o;
    o.xv = dn_v4<V4>(m[0] / b[0], m[1] / b[1], m[2] / b[2], V);
    o.nz = dn_v4<V4>(f[4], f[5], f[6], f[7]);
    o.gb = dn_v4<V4>(g, b[0], b[1], b[2]);
    if (U) {
        if (k >= 1) {
            const float n = (float)k;
            o.un = dn_v4<V4>((a[3] / n) / (b[0] * b[0]), (a[4] / n) / (b[1] * b[1]), (a[5] / n) / (b[2] * b[2]), n);
        } else {
            o.un = dn_v4<V4>(0.f, 0.f, 0.f, 0.f);
        }
    }
    return o;
}

// The spatial estimate at pixel (x, y): the V that level 0 reads.  src.xv / src.un / src.nz(qx, qy) give
// prepare's planes at an in-frame pixel, g is the pixel's depth slope.  A pixel with 1 <= k < minCount
// pools the moments of its (2R+1)^2 neighbours, each weighted by its count times the filter's normal and
// depth edge-stops at step 1 (no luminance term: this variance is what that term divides by); any other
// pixel, and one whose kept taps hold fewer than two samples, keeps prepare's V.  A tap outside the
// frame is skipped; a tap without a sample, with a sum that is not finite, or whose e is not below 16
// (NaN included) is dropped: it adds to no sum.
template <int R, class Src>
PBR_HD float dn_estimate(int W, int H, int x, int y, int minCount, float in, float iz, float g, const Src& src) {
    const auto cp = src.xv(x, y);
    const float n = src.un(x, y).w;
    if (!(n >= 1.f && n < (float)minCount)) return cp.w;
    const auto np = src.nz(x, y);
    const float zc = 1e-3f * np.w + 1e-6f;
    float sa = 0.f, s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f};
    int kt = 0;   // the samples behind the kept taps, saturating: only kt < 2 is asked
#pragma unroll
    for (int j = -R; j <= R; ++j) {
        // (unsigned: a row above the frame wraps past H)
        const unsigned qy = (unsigned)y + (unsigned)j;
        if (qy >= (unsigned)H) continue;
#pragma unroll
        for (int i = -R; i <= R; ++i) {
            const unsigned qx = (unsigned)x + (unsigned)i;
            if (qx >= (unsigned)W) continue;
            const auto uq = src.un((int)qx, (int)qy);
            if (!(uq.w >= 1.f)) continue;
            const auto cq = src.xv((int)qx, (int)qy);
            if (!(dn_finite(cq.x) && dn_finite(cq.y) && dn_finite(cq.z) && dn_finite(uq.x) && dn_finite(uq.y) && dn_finite(uq.z)))
                continue;
            float w = 1.f;
            if (i != 0 || j != 0) {
                const int ai = i < 0 ? -i : i, aj = j < 0 ? -j : j;
                const auto nq = src.nz((int)qx, (int)qy);
                const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                const float en = ((dx * dx + dy * dy) + dz * dz) * in;
                const float dd = np.w - nq.w;
                const float den = g * (float)(ai > aj ? ai : aj) + zc;
                const float ez = ((dd * dd) / (den * den)) * iz;
                const float e = en + ez;
                if (!(e < 16.f)) continue;
                float t = 1.f - e * 0.0625f;
                t = t * t;
                t = t * t;
                t = t * t;
                t = t * t;
                w = t;
            }
            const float a = w * uq.w;
            sa = sa + a;
            s1[0] = s1[0] + a * cq.x;
            s1[1] = s1[1] + a * cq.y;
            s1[2] = s1[2] + a * cq.z;
            s2[0] = s2[0] + a * uq.x;
            s2[1] = s2[1] + a * uq.y;
            s2[2] = s2[2] + a * uq.z;
            kt = kt + (kt < 2 ? (uq.w >= 2.f ? 2 : 1) : 0);
        }
    }
    if (kt < 2) return cp.w;
    float sig[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float M = s1[c] / sa, Um = s2[c] / sa;
        const float d = Um - M * M;
        sig[c] = d > 0.f ? d : 0.f;
    }
    return ((sig[0] + sig[1]) + sig[2]) / n;
}

// What is wrong with a denoise call's parameters (nullptr: nothing); shared by the device and the host
// entry.  sv == NULL: the plain call, which needs two samples for a variance.
inline const char* dn_params_error(const pbr_denoise* p, const pbr_spatial_variance* sv, int samples, const int32_t* counts) {
    if (!p) return "denoise: null parameters";
    if (p->width < 1 || p->height < 1) return "denoise: width and height must be >= 1";
    if ((long long)p->width * p->height >= (1ll << 31)) return "denoise: width * height must be below 2^31";
    if (p->iterations < 1 || p->iterations > 8) return "denoise: iterations must be 1..8";
    if (!(p->sigma_l > 0.f) || !(p->sigma_n > 0.f) || !(p->sigma_z > 0.f)) return "denoise: sigma_l, sigma_n and sigma_z must be > 0";
    if (!sv) {
        if (!counts && samples < 2) return "denoise: samples must be >= 2 (or give per-pixel counts)";
        return nullptr;
    }
    if (sv->min_count < 2 || sv->min_count > 64) return "denoise: the spatial estimate's min_count must be 2..64";
    if (sv->radius < 1 || sv->radius > 3) return "denoise: the spatial estimate's radius must be 1..3";
    if (!counts && samples < 1) return "denoise: samples must be >= 1 (or give per-pixel counts)";
    return nullptr;
}

}  // namespace pbr
