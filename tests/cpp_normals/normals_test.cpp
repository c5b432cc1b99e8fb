// normals_test.cpp — a TriangleMesh with per-vertex normals (mesh->n) through the C++ host API
// (include/pbr/pbr.h): it uploads, renders, and Scene::Intersect returns the smooth shading frame.
//
//   normals_test gpu [file]   builds the tent mesh below with N under Translate * Scale, renders a small
//                             Whitted frame, and intersects rays; with `file` (per ray 16 float32: the ray's
//                             7 floats, then n, shading.n and shading.dpdu of pbr_hip_query's record for the
//                             same scene built through the Python layer, written by tests/test_host_normals.py)
//                             the rays are the file's and the interactions equal its records bit for bit
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pbr/pbr.h"

using namespace PBR;

namespace {

int failures = 0;
void expect(bool ok, const std::string& what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++failures;
}

// The tent: four vertices, two triangles, normals leaning outwards (tests/test_host_normals.py holds the
// same numbers).  Every transform entry is exact in float, so both layers bake the same bits.
const Point3f kP[4] = {Point3f(-1.f, 0.f, 1.f), Point3f(1.f, 0.f, 1.f), Point3f(1.f, 0.5f, -1.f), Point3f(-1.f, 0.25f, -1.f)};
const int kI[6] = {0, 1, 2, 0, 2, 3};
const Normal3f kN[4] = {Normal3f(-0.25f, 1.f, 0.25f), Normal3f(0.25f, 1.f, 0.25f), Normal3f(0.25f, 1.f, -0.125f),
                        Normal3f(-0.25f, 1.f, -0.25f)};

int run_gpu(const char* dump) {
    const int W = 24, H = 16;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    const Transform o2w = Translate(Vector3f(0.25f, -0.5f, 0.f)) * Scale(2.f, 1.f, 0.5f);
    const Transform w2o = Inverse(o2w);
    auto matte = std::make_shared<MatteMaterial>(std::make_shared<ConstantTexture<Spectrum>>(Spectrum(0.6f)),
                                                 std::make_shared<ConstantTexture<float>>(0.f), nullptr);
    std::vector<std::shared_ptr<Primitive>> prims;
    const auto shapes = CreateTriangleMesh(&o2w, &w2o, false, 2, kI, 4, kP, nullptr, kN, nullptr);
    for (auto& s : shapes) prims.push_back(std::make_shared<GeometricPrimitive>(s, matte, nullptr, MediumInterface()));
    auto* tri = dynamic_cast<const Triangle*>(shapes[0].get());
    expect(tri && tri->mesh->n.size() == 12, "TriangleMesh keeps its N");
    std::vector<std::shared_ptr<Light>> lights;
    lights.push_back(std::make_shared<PointLight>(Translate(Vector3f(0.f, 4.f, 2.f)), MediumInterface(), Spectrum(20.f)));
    Scene scene(std::make_shared<BVHAccel>(prims, 1), lights);
    Transform lookat = LookAt(Point3f(0.f, 3.f, 4.f), Point3f(0.f, 0.f, 0.f), Vector3f(0.f, 1.f, 0.f));
    std::shared_ptr<Camera> cam(CreatePerspectiveCamera(W, H, Inverse(lookat), nullptr));
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    WhittedIntegrator integ(5, cam, std::make_shared<HaltonSampler>(4, bounds), bounds, &fb);
    double seconds = 0;
    integ.Render(scene, seconds);   // (a mesh with N used to be refused at the upload this triggers)
    expect(true, "a scene whose mesh has N renders");

    std::vector<float> rec;
    if (dump) {
        FILE* f = std::fopen(dump, "rb");
        float v[16];
        while (f && std::fread(v, sizeof(float), 16, f) == 16) rec.insert(rec.end(), v, v + 16);
        if (f) std::fclose(f);
        expect(!rec.empty(), std::string("read ") + dump);
    } else {   // no file: rays of its own, checked for what a smooth frame implies
        const float t[3][2] = {{0.3f, 0.2f}, {-0.9f, 0.1f}, {1.2f, -0.3f}};
        for (auto& q : t) {
            const float v[16] = {q[0], 3.f, q[1], 0.f, -1.f, 0.f, INFINITY};
            rec.insert(rec.end(), v, v + 16);
        }
    }
    const size_t n = rec.size() / 16;
    int hits = 0, bad = 0, smooth = 0;
    for (size_t i = 0; i < n; ++i) {
        const float* v = &rec[16 * i];
        Ray r(Point3f(v[0], v[1], v[2]), Vector3f(v[3], v[4], v[5]), v[6]);
        SurfaceInteraction si;
        if (!scene.Intersect(r, &si)) continue;
        ++hits;
        const float got[9] = {si.n.x, si.n.y, si.n.z, si.shading.n.x, si.shading.n.y, si.shading.n.z,
                              si.shading.dpdu.x, si.shading.dpdu.y, si.shading.dpdu.z};
        if (dump && std::memcmp(got, v + 7, sizeof got) != 0) {
            if (!bad) std::printf("     ray %zu: shading.n (%g %g %g), the record's (%g %g %g)\n", i, got[3], got[4], got[5], v[10], v[11], v[12]);
            ++bad;
        }
        const float d = si.n.x * si.shading.n.x + si.n.y * si.shading.n.y + si.n.z * si.shading.n.z;
        if (d > 0.f && d < 0.99999f) ++smooth;   // shading.n is not the facet normal, and n lies on its side
    }
    expect(hits >= 3, "the rays hit the mesh (" + std::to_string(hits) + " of " + std::to_string(n) + ")");
    expect(smooth == hits, "shading.n is the interpolated normal, with n on its side");
    if (dump) expect(bad == 0, "n, shading.n and shading.dpdu equal the C-ABI records bit for bit");
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        const int rc = run_gpu(argc > 2 ? argv[2] : nullptr);
        std::printf("%d failure(s)\n", failures);
        return rc;
    } catch (const std::exception& e) {
        std::printf("FAIL uncaught: %s\n", e.what());
        return 2;
    }
}
