// pbr_quad_order.h — the visit order of a quad node's four slots, for the packet walk
// (pbr_device.h traverse_packet) and, compiled for the host, tests/cpp_quad_order.
//
// A quad node stands for binary node N and holds, in slot columns 0..3, the children of N's first
// child A (columns 0, 1) and of its second child B (columns 2, 3); meta carries the split axes of N,
// A and B (pbr_scene.cpp build_quad_nodes).  BVHAccel visits the near child of a split first, near
// being the second child when the ray's direction is negative on the split axis.  So a ray of sign
// octant oct (bit a set: direction negative on axis a) visits the columns in the order
//   sN = (oct >> axN) & 1, sA = (oct >> axA) & 1, sB = (oct >> axB) & 1
//   col_hi = pos_hi ^ sN,  col_lo = pos_lo ^ (col_hi ? sB : sA)
// which is what quad_order's swaps (pairs by sA and sB, then halves by sN) produce.
#pragma once
#include "pbr_math.h"

namespace pbr {

struct QuadSigns { int sN, sA, sB; };

// meta = axN | axA << 2 | axB << 4 | validMask << 8, axes 0..2
PBR_HD QuadSigns quad_signs(int meta, int oct) {
    QuadSigns s;
    s.sN = (oct >> (meta & 3)) & 1;
    s.sA = (oct >> ((meta >> 2) & 3)) & 1;
    s.sB = (oct >> ((meta >> 4) & 3)) & 1;
    return s;
}

// visit position 0..3 → slot column
PBR_HD int quad_col(QuadSigns s, int pos) {
    const int hi = (pos >> 1) ^ s.sN;
    return hi * 2 + ((pos & 1) ^ (hi ? s.sB : s.sA));
}

// Four per-column values into visit order: v[pos] = v[quad_col(s, pos)], by three conditional swaps
// (the pair inside each half by sA / sB, then the halves by sN).
template <class T>
PBR_HD void quad_visit_order(QuadSigns s, T (&v)[4]) {
    const bool cA = s.sA != 0, cB = s.sB != 0, cN = s.sN != 0;
    const T a0 = cA ? v[1] : v[0], a1 = cA ? v[0] : v[1];
    const T b0 = cB ? v[3] : v[2], b1 = cB ? v[2] : v[3];
    v[0] = cN ? b0 : a0; v[1] = cN ? b1 : a1;
    v[2] = cN ? a0 : b0; v[3] = cN ? a1 : b1;
}

// Bit pos set: the value at visit position pos (m in visit order) is not zero — some lane passes.
template <class T>
PBR_HD int quad_nonzero(const T (&m)[4]) {
    return (int)(m[0] != 0) | (int)(m[1] != 0) << 1 | (int)(m[2] != 0) << 2 | (int)(m[3] != 0) << 3;
}

// The position a node step enters: the first one set in quad_nonzero's bits, -1 when none is.
PBR_HD int quad_first(int some) {
    return (some & 1) ? 0 : ((some & 2) ? 1 : ((some & 4) ? 2 : ((some & 8) ? 3 : -1)));
}

// The entries a node step pushes after entering the first position: the later positions set in
// `some`, far-last — push(position, column, value) for positions 3, 2, 1.
template <class T, class F>
PBR_HD void quad_push_later(QuadSigns s, int some, const T (&m)[4], F&& push) {
    const int later = some & (some - 1);   // without the lowest set bit, the entered position
    if (later & 8) push(3, quad_col(s, 3), m[3]);
    if (later & 4) push(2, quad_col(s, 2), m[2]);
    if (later & 2) push(1, quad_col(s, 1), m[1]);
}

}  // namespace pbr
