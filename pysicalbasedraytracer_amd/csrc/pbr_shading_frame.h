// pbr_shading_frame.h — the shading frame of a triangle whose mesh has per-vertex normals
// (Triangle.cpp:186-253 and SurfaceInteraction::SetShadingGeometry, Interaction.cpp:98-113), for the
// device's triangle_si and, compiled for the host, pbr_hip_shading_host.  mesh->s is not carried by
// the descriptor, and dndu / dndv have no reader here.
#pragma once
#include "pbr_math.h"

namespace pbr {

struct ShadingFrame { f3 n, sn, dpdu; };

// n0 n1 n2: the vertices' world-space normals (not unit length after a non-rigid transform);
// n: the geometric normal, already flipped by reverseOrientation ^ transformSwapsHandedness;
// dpdu: Triangle::Intersect's, (0,0,0) on a degenerate UV map; reverse: the shape's own
// reverseOrientation.  The operations and their order are the reference's:
//   ns = b0 n0 + b1 n1 + b2 n2, normalised, or n when its squared length is not above 0
//   ss = Normalize(dpdu)                                  (NaN when dpdu is zero)
//   ts = Cross(ss, ns); squared length above 0: ts = Normalize(ts), ss = Cross(ts, ns)
//                       else (zero or NaN):     CoordinateSystem(ns, &ss, &ts)
//   reverse: ts = -ts
//   shading.n = Normalize(Cross(ss, ts)); n = Faceforward(n, shading.n); shading.dpdu = ss
PBR_HD ShadingFrame shading_frame(f3 n0, f3 n1, f3 n2, float b0, float b1, float b2, f3 n, f3 dpdu, bool reverse) {
    f3 ns = b0 * n0 + b1 * n1 + b2 * n2;
    if (len2(ns) > 0) ns = normalize(ns);
    else ns = n;
    f3 ss = normalize(dpdu);
    f3 ts = cross(ss, ns);
    if (len2(ts) > 0.f) {
        ts = normalize(ts);
        ss = cross(ts, ns);
    } else {
        coordinate_system(ns, &ss, &ts);
    }
    if (reverse) ts = -ts;
    ShadingFrame f;
    f.sn = normalize(cross(ss, ts));
    f.n = faceforward(n, f.sn);
    f.dpdu = ss;
    return f;
}

// Triangle::Sample's normal of a point on a mesh with normals (Triangle.cpp:372-376): the geometric
// normal of Cross(p1 - p0, p2 - p0), turned to the side of the interpolated normal, which is not
// normalised.  The third weight is the sample's own 1 - b0 - b1.
PBR_HD f3 sampled_normal(f3 n0, f3 n1, f3 n2, float b0, float b1, f3 n) {
    const f3 ns = b0 * n0 + b1 * n1 + (1 - b0 - b1) * n2;
    return faceforward(n, ns);
}

// Triangle::Intersect's dpdu and geometric normal (Triangle.cpp:148-184), the two inputs above that
// triangle_si (pbr_device.h) forms on the way: the same lines, for the host entry point
// pbr_hip_shading_host.  uv: the three vertices' (u, v); flip: reverseOrientation ^ swapsHandedness.
PBR_HD void triangle_frame_inputs(f3 p0, f3 p1, f3 p2, const float* uv, bool flip, f3* n, f3* dpdu) {
    const float d02x = uv[0] - uv[4], d02y = uv[1] - uv[5], d12x = uv[2] - uv[4], d12y = uv[3] - uv[5];
    const f3 dp02 = p0 - p2, dp12 = p1 - p2;
    const float determinant = d02x * d12y - d02y * d12x;
    const bool degenerate = (double)fabsf(determinant) < 1e-8;
    *dpdu = mk(0, 0, 0);
    if (!degenerate) {
        const float invdet = 1 / determinant;
        *dpdu = (d12y * dp02 - d02y * dp12) * invdet;
    }
    *n = normalize(cross(dp02, dp12));
    if (flip) *n = -*n;
}

}  // namespace pbr
