// pbr_slab.h — the slab test of a quad slot's box, for the quad walks (pbr_device.h slab_nf,
// slab_nf_lanes) and, compiled for the host, tests/cpp_slab.
//
// Bounds3::IntersectP (Geometry.h:1438-1468) on the box's near and far planes (near = the plane the
// ray enters through: hi on an axis where the direction is negative, lo otherwise) is
//   tMin = (nr.x − o.x)·inv.x, tMax = (fr.x − o.x)·inv.x, the same for y and z;
//   reject if tMin > tyMax or tyMin > tMax;  tMin = tyMin > tMin ? tyMin : tMin;  tMax likewise;
//   reject if tMin > tzMax or tzMin > tMax;  the z selects;  accept iff tMin < ray.tMax and tMax > 0.
// slab_exact is that sequence.  slab_fold takes the largest near value and the smallest far value with
// fmax / fmin (v_max3_f32 / v_min3_f32) and compares them once.
//
// The two agree — the same decision, and tMin the same number — for a ray whose three inv components
// are finite and not zero and whose origin is finite (slab_ray_foldable) against a box whose planes
// are finite with lo ≤ hi on every axis (slab_box_foldable):
//   * no product is 0·∞, so no value is NaN;
//   * on each axis near value ≤ far value: subtracting a common o is monotone under correct rounding,
//     and so is multiplying by a common factor (order-reversing for a negative one, which is the axis
//     where near and far planes are swapped), overflow to ±∞ included;
//   * the four rejections test the six cross-axis pairs tiMin ≤ tjMax; with the three same-axis pairs
//     given, all nine hold exactly when max(tiMin) ≤ min(tjMax);
//   * the select chains and fmax / fmin pick the same numbers; only the sign of a zero can differ, and
//     every use of tMin and tMax is a comparison.
// Outside that class (a zero direction component makes inv ±∞ and, with the origin on the plane, a
// NaN) the forms differ: a select keeps its old value against a NaN, fmax / fmin drop the NaN.  Such
// rays, and scenes with such boxes, take slab_exact.
#pragma once
#include "pbr_math.h"
#include <stddef.h>

namespace pbr {

struct Slab {
    float tMin, tMax;   // the entry and exit distances (meaningful where `order` holds)
    bool order;         // no axis' near value lies beyond another's far value
    bool ahead;         // tMax > 0
    bool within;        // tMin < ray.tMax
};

// The reference's sequence.  stage (optional): the first of its four rejections that fires, 1..4
// (tMin > tyMax, tyMin > tMax, tMin > tzMax, tzMin > tMax), 0 when none does.
PBR_HD Slab slab_exact(float nx, float ny, float nz, float fx, float fy, float fz, float ox, float oy, float oz,
                       float ix, float iy, float iz, float rayTMax, int* stage = nullptr) {
    float tMin = (nx - ox) * ix;
    float tMax = (fx - ox) * ix;
    const float tyMin = (ny - oy) * iy;
    const float tyMax = (fy - oy) * iy;
    const float tzMin = (nz - oz) * iz;
    const float tzMax = (fz - oz) * iz;
    const bool r1 = tMin > tyMax, r2 = tyMin > tMax;
    tMin = tyMin > tMin ? tyMin : tMin;
    tMax = tyMax < tMax ? tyMax : tMax;
    const bool r3 = tMin > tzMax, r4 = tzMin > tMax;
    tMin = tzMin > tMin ? tzMin : tMin;
    tMax = tzMax < tMax ? tzMax : tMax;
    if (stage) *stage = r1 ? 1 : (r2 ? 2 : (r3 ? 3 : (r4 ? 4 : 0)));
    return Slab{tMin, tMax, !(r1 | r2 | r3 | r4), tMax > 0, tMin < rayTMax};
}

// The folded form: 12 arithmetic operations, one three-way max, one three-way min, three comparisons.
PBR_HD Slab slab_fold(float nx, float ny, float nz, float fx, float fy, float fz, float ox, float oy, float oz,
                      float ix, float iy, float iz, float rayTMax) {
    const float txMin = (nx - ox) * ix;
    const float txMax = (fx - ox) * ix;
    const float tyMin = (ny - oy) * iy;
    const float tyMax = (fy - oy) * iy;
    const float tzMin = (nz - oz) * iz;
    const float tzMax = (fz - oz) * iz;
    const float tMin = __builtin_fmaxf(__builtin_fmaxf(txMin, tyMin), tzMin);
    const float tMax = __builtin_fminf(__builtin_fminf(txMax, tyMax), tzMax);
    return Slab{tMin, tMax, !(tMin > tMax), tMax > 0, tMin < rayTMax};
}

// finite: neither ±∞ nor NaN
PBR_HD bool slab_finite(float v) { return (fbits(v) & 0x7fffffffu) < 0x7f800000u; }

// The ray's half of the guarantee: inv = 1 / direction, per component.
PBR_HD bool slab_ray_foldable(float ox, float oy, float oz, float ix, float iy, float iz) {
    return slab_finite(ix) && ix != 0.f && slab_finite(iy) && iy != 0.f && slab_finite(iz) && iz != 0.f &&
           slab_finite(ox) && slab_finite(oy) && slab_finite(oz);
}

// The scene's half: every valid slot of every quad node (32 floats each: rows lo.x/y/z, hi.x/y/z of
// the four slots, the references, meta with the valid mask in bits 8..11) has finite planes with
// lo ≤ hi on all axes.  What an invalid slot holds does not matter: it is never tested.
PBR_HD bool slab_box_foldable(const float* lo, const float* hi) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = ok && slab_finite(lo[a]) && slab_finite(hi[a]) && lo[a] <= hi[a];
    return ok;
}
inline bool slab_scene_foldable(const float* quad, size_t nQuad) {
    for (size_t q = 0; q < nQuad; ++q) {
        const float* w = quad + 32 * q;
        const uint32_t meta = fbits(w[28]);
        for (int s = 0; s < 4; ++s) {
            if (!((meta >> (8 + s)) & 1)) continue;
            const float lo[3] = {w[s], w[4 + s], w[8 + s]}, hi[3] = {w[12 + s], w[16 + s], w[20 + s]};
            if (!slab_box_foldable(lo, hi)) return false;
        }
    }
    return true;
}

}  // namespace pbr
