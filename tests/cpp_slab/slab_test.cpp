// The quad walks' slab test (pysicalbasedraytracer_amd/csrc/pbr_slab.h) compiled for the host: the
// reference's sequence (slab_exact) against the folded form (slab_fold), and the two predicates that
// decide where the folded form may run.  tests/test_host_slab.py drives it.
//
//   slab_test equal N SEED   N seeded box/ray pairs, foldable rays against ordered finite boxes: one
//                            line of counts (see main)
//   slab_test guard N SEED   N pairs per class of non-foldable rays: per class, how many pairs the
//                            two forms decide differently
//   slab_test rays FILE      FILE = float32 records (o.x o.y o.z inv.x inv.y inv.z): slab_ray_foldable
//                            of each, one digit per line
//   slab_test scene FILE     FILE = float32 quad nodes, 32 floats each: slab_scene_foldable, one digit
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pbr_slab.h"

using namespace pbr;

namespace {

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    float u() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }   // [0, 1)
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(float p) { return u() < p; }
};

const float kInf = std::numeric_limits<float>::infinity();

struct Case {
    float lo[3], hi[3], o[3], d[3], tMax;
};

// a coordinate at scale s: on a grid of halves, or anywhere in [-8, 8) s
float coord(Rng& g, float s, bool grid) { return grid ? s * 0.5f * (float)(g.below(33) - 16) : s * (g.u() * 16.f - 8.f); }

// A box and a ray aimed at a point of the box grown threefold, so that hits and every kind of miss
// occur.  Seven decades of scale; a tenth of the boxes flat per axis; 15% of the origins on a plane of
// the box; directions raw, snapped to ±1 / ±½, or with one component down to 1e-30.
Case make_case(Rng& g) {
    Case c;
    const float s = std::pow(10.f, (float)(g.below(7) - 3));
    const bool grid = g.chance(0.5f);
    for (int a = 0; a < 3; ++a) {
        c.lo[a] = coord(g, s, grid);
        const float e = g.chance(0.1f) ? 0.f : (grid ? s * 0.5f * (float)(1 + g.below(8)) : s * 4.f * g.u());
        c.hi[a] = c.lo[a] + e;
        c.o[a] = coord(g, s, grid) * 1.5f;
    }
    if (g.chance(0.15f)) {
        const int a = g.below(3);
        c.o[a] = g.chance(0.5f) ? c.lo[a] : c.hi[a];
    }
    float target[3];
    for (int a = 0; a < 3; ++a) target[a] = c.lo[a] + (c.hi[a] - c.lo[a]) * (g.u() * 3.f - 1.f) + (grid ? 0.f : s * (g.u() - 0.5f));
    for (int a = 0; a < 3; ++a) c.d[a] = target[a] - c.o[a];
    if (g.chance(0.15f)) for (int a = 0; a < 3; ++a) c.d[a] = -c.d[a];   // the box behind the ray
    const float kind = g.u();
    if (kind < 0.2f) {
        for (int a = 0; a < 3; ++a) c.d[a] = (c.d[a] < 0 ? -1.f : 1.f) * (g.chance(0.5f) ? 1.f : 0.5f);
    } else if (kind < 0.35f) {
        const int a = g.below(3);
        c.d[a] = (g.chance(0.5f) ? -1.f : 1.f) * std::pow(10.f, -30.f * g.u());
    } else if (kind < 0.5f) {
        const float k = std::pow(10.f, 6.f * g.u() - 3.f);
        for (int a = 0; a < 3; ++a) c.d[a] *= k;
    }
    c.tMax = kInf;
    return c;
}

struct Planes { float n[3], f[3], inv[3]; };
Planes planes(const Case& c) {   // near = the plane the ray enters through, as the walks pick it
    Planes p;
    for (int a = 0; a < 3; ++a) {
        p.inv[a] = 1.f / c.d[a];
        const bool neg = p.inv[a] < 0;
        p.n[a] = neg ? c.hi[a] : c.lo[a];
        p.f[a] = neg ? c.lo[a] : c.hi[a];
    }
    return p;
}
Slab exact(const Case& c, const Planes& p, int* stage) {
    return slab_exact(p.n[0], p.n[1], p.n[2], p.f[0], p.f[1], p.f[2], c.o[0], c.o[1], c.o[2], p.inv[0], p.inv[1], p.inv[2], c.tMax, stage);
}
Slab fold(const Case& c, const Planes& p) {
    return slab_fold(p.n[0], p.n[1], p.n[2], p.f[0], p.f[1], p.f[2], c.o[0], c.o[1], c.o[2], p.inv[0], p.inv[1], p.inv[2], c.tMax);
}
bool decision(const Slab& s) { return s.order && s.ahead && s.within; }

int run_equal(long n, uint64_t seed) {
    Rng g{seed};
    long cases = 0, resampled = 0, accept = 0, stage[5] = {0, 0, 0, 0, 0}, behind = 0, beyond = 0;
    long diffDecision = 0, diffPredicate = 0, diffTMin = 0, diffTMinAccepted = 0, diffTMax = 0;
    while (cases < n) {
        Case c = make_case(g);
        Planes p = planes(c);
        const float lo[3] = {c.lo[0], c.lo[1], c.lo[2]}, hi[3] = {c.hi[0], c.hi[1], c.hi[2]};
        if (!slab_ray_foldable(c.o[0], c.o[1], c.o[2], p.inv[0], p.inv[1], p.inv[2]) || !slab_box_foldable(lo, hi)) {
            ++resampled;
            continue;
        }
        // ray.tMax: infinite, or around the entry distance — at it, one ulp either side, anywhere near
        int st = 0;
        const Slab probe = exact(c, p, &st);
        if (g.chance(0.5f) && probe.tMin > 0 && probe.tMin < kInf) {
            const int k = g.below(4);
            c.tMax = k == 0 ? probe.tMin : (k == 1 ? std::nextafter(probe.tMin, kInf) : (k == 2 ? std::nextafter(probe.tMin, 0.f) : probe.tMin * (0.5f + g.u())));
        }
        const Slab e = exact(c, p, &st), f = fold(c, p);
        ++cases;
        ++stage[st];
        if (st == 0 && !e.ahead) ++behind;
        if (st == 0 && e.ahead && !e.within) ++beyond;
        if (decision(e)) ++accept;
        if (decision(e) != decision(f)) ++diffDecision;
        if (e.order != f.order || e.ahead != f.ahead || e.within != f.within) ++diffPredicate;
        if (!(e.tMin == f.tMin)) ++diffTMin;
        if (!(e.tMax == f.tMax)) ++diffTMax;
        if (decision(e) && !(e.tMin == f.tMin)) ++diffTMinAccepted;
    }
    std::printf("cases %ld resampled %ld accept %ld stage1 %ld stage2 %ld stage3 %ld stage4 %ld behind %ld beyond %ld "
                "diff_decision %ld diff_predicate %ld diff_tmin %ld diff_tmin_accepted %ld diff_tmax %ld\n",
                cases, resampled, accept, stage[1], stage[2], stage[3], stage[4], behind, beyond, diffDecision, diffPredicate, diffTMin,
                diffTMinAccepted, diffTMax);
    return 0;
}

// Non-foldable rays: one direction component is +0 or −0 (zero), a denormal (denormal), or ±0 with
// the origin on one of the box's planes of that axis (on_plane: 0·∞ = NaN).
int run_guard(long n, uint64_t seed) {
    Rng g{seed};
    const char* names[3] = {"zero", "denormal", "on_plane"};
    for (int cls = 0; cls < 3; ++cls) {
        long differ = 0, foldable = 0, nan = 0;
        for (long i = 0; i < n; ++i) {
            Case c = make_case(g);
            const int a = g.below(3);
            const float sign = g.chance(0.5f) ? -1.f : 1.f;
            c.d[a] = cls == 1 ? sign * 1e-39f * (0.1f + g.u()) : sign * 0.f;
            for (int b = 0; b < 3; ++b)
                if (b != a && c.d[b] == 0.f) c.d[b] = 1.f;
            if (cls == 2) c.o[a] = g.chance(0.5f) ? c.lo[a] : c.hi[a];
            const Planes p = planes(c);
            if (slab_ray_foldable(c.o[0], c.o[1], c.o[2], p.inv[0], p.inv[1], p.inv[2])) ++foldable;
            int st;
            const Slab e = exact(c, p, &st), f = fold(c, p);
            if (e.tMin != e.tMin || e.tMax != e.tMax) ++nan;
            if (decision(e) != decision(f)) ++differ;
        }
        std::printf("%s cases %ld foldable %ld nan %ld differ %ld\n", names[cls], n, foldable, nan, differ);
    }
    return 0;
}

bool read_floats(const char* path, std::vector<float>* v) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    float buf[1024];
    size_t k;
    while ((k = std::fread(buf, sizeof(float), 1024, f)) > 0) v->insert(v->end(), buf, buf + k);
    std::fclose(f);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "equal")) return run_equal(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
    if (argc == 4 && !std::strcmp(argv[1], "guard")) return run_guard(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
    std::vector<float> v;
    if (argc == 3 && !std::strcmp(argv[1], "rays") && read_floats(argv[2], &v) && v.size() % 6 == 0) {
        for (size_t i = 0; i < v.size(); i += 6) std::printf("%d\n", (int)slab_ray_foldable(v[i], v[i + 1], v[i + 2], v[i + 3], v[i + 4], v[i + 5]));
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "scene") && read_floats(argv[2], &v) && v.size() % 32 == 0) {
        std::printf("%d\n", (int)slab_scene_foldable(v.data(), v.size() / 32));
        return 0;
    }
    std::fprintf(stderr, "usage: slab_test equal|guard N SEED | rays|scene FILE\n");
    return 2;
}
