// follow_test.cpp — SamplerIntegrator::RenderFeatures with mirrorBounces (include/pbr/pbr.h): the feature
// pass that follows mirror bounces, through the C++ host API.
//
//   follow_test cpu                 no GPU needed: a mirrorBounces outside 0..16 throws std::invalid_argument
//                                   before any device call
//   follow_test gpu [file0 file2]   the default argument equals mirrorBounces = 0 and differs from 2; with the
//                                   files (40·30·8 float32 each: the C-ABI images of the same frame with 0 and 2
//                                   bounces, written by tests/test_host_follow.py) the buffers equal them
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

std::shared_ptr<Texture<Spectrum>> rgbTex(float r, float g, float b) {
    float v[3] = {r, g, b};
    return std::make_shared<ConstantTexture<Spectrum>>(Spectrum::FromRGB(v));
}
std::shared_ptr<Texture<float>> fTex(float v) { return std::make_shared<ConstantTexture<float>>(v); }

struct Built {
    std::vector<std::unique_ptr<Transform>> xf;   // shapes keep raw Transform pointers
    std::unique_ptr<Scene> scene;
    std::shared_ptr<Camera> cam;
};
const Transform* keep(Built& b, const Transform& t) {
    b.xf.push_back(std::make_unique<Transform>(t));
    return b.xf.back().get();
}

// Two mirror balls either side of a matte one, radius 1.5 each, under a point light, seen from z = 7
// (tests/test_host_follow.py builds the same scene through the Python layer): the mirrors show the matte
// ball, each other, and nothing.
void build_balls(Built& b, int W, int H) {
    std::vector<std::shared_ptr<Primitive>> prims;
    auto ball = [&](float x, const std::shared_ptr<Material>& m) {
        const Transform* o2w = keep(b, Translate(Vector3f(x, 0.f, 0.f)));
        const Transform* w2o = keep(b, Inverse(*o2w));
        prims.push_back(std::make_shared<GeometricPrimitive>(std::make_shared<Sphere>(o2w, w2o, false, 1.5f), m, nullptr, MediumInterface()));
    };
    ball(0.f, std::make_shared<MatteMaterial>(rgbTex(0.5f, 0.75f, 0.25f), fTex(0.f), nullptr));
    ball(-3.25f, std::make_shared<MirrorMaterial>(rgbTex(0.5f, 1.f, 0.25f), nullptr));
    ball(3.25f, std::make_shared<MirrorMaterial>(rgbTex(1.f, 0.5f, 0.5f), nullptr));
    std::vector<std::shared_ptr<Light>> lights;
    lights.push_back(std::make_shared<PointLight>(Translate(Vector3f(0.f, 4.f, 4.f)), MediumInterface(), Spectrum(20.f)));
    b.scene = std::make_unique<Scene>(std::make_shared<BVHAccel>(prims, 1), lights);
    Transform lookat = LookAt(Point3f(0.f, 0.f, 7.f), Point3f(0.f, 0.f, 0.f), Vector3f(0.f, 1.f, 0.f));
    b.cam = std::shared_ptr<Camera>(CreatePerspectiveCamera(W, H, Inverse(lookat), nullptr));
}

template <class Fn> bool throws_invalid(Fn fn) {
    try {
        fn();
    } catch (const std::invalid_argument& e) {
        std::printf("     (%s)\n", e.what());
        return std::string(e.what()).find("mirrorBounces") != std::string::npos;
    }
    return false;
}

bool same(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}
bool same(const FeatureBuffers& a, const FeatureBuffers& b) {
    return a.width == b.width && a.height == b.height && same(a.albedo, b.albedo) && same(a.normal, b.normal) &&
           same(a.depth, b.depth) && same(a.coverage, b.coverage);
}

int run_cpu() {
    const int W = 32, H = 24;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_balls(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    FeatureBuffers out;
    auto halton = [&] { return std::make_shared<WhittedIntegrator>(5, b.cam, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb); };
    // (a device call would throw std::runtime_error where there is no GPU, and return normally where there is one)
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, 0, 2, &out, 17); }), "mirrorBounces above 16 is refused");
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, 0, 2, &out, -1); }), "a negative mirrorBounces is refused");
    return failures ? 1 : 0;
}

bool equals_image(const char* path, const FeatureBuffers& f, int W, int H) {
    std::vector<float> img((size_t)W * H * 8);
    FILE* fp = std::fopen(path, "rb");
    const size_t got = fp ? std::fread(img.data(), sizeof(float), img.size(), fp) : 0;
    if (fp) std::fclose(fp);
    expect(got == img.size(), std::string("read ") + path);
    bool eq = got == img.size();
    for (size_t p = 0; eq && p < (size_t)W * H; ++p)
        eq = std::memcmp(&img[8 * p], &f.albedo[3 * p], 12) == 0 && std::memcmp(&img[8 * p + 3], &f.coverage[p], 4) == 0 &&
             std::memcmp(&img[8 * p + 4], &f.normal[3 * p], 12) == 0 && std::memcmp(&img[8 * p + 7], &f.depth[p], 4) == 0;
    return eq;
}

int run_gpu(const char* dump0, const char* dump2) {
    const int W = 40, H = 30, spp = 8;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_balls(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    auto make = [&] { return std::make_shared<PathIntegrator>(8, b.cam, std::make_shared<HaltonSampler>(spp, bounds), bounds, 0.8f, "uniform", &fb); };
    FeatureBuffers plain, zero, two, cut;
    make()->RenderFeatures(*b.scene, 0, 8, &plain);
    make()->RenderFeatures(*b.scene, 0, 8, &zero, 0);
    make()->RenderFeatures(*b.scene, 0, 8, &two, 2);
    expect(same(plain, zero), "the default argument is mirrorBounces = 0");
    expect(same(plain.coverage, two.coverage), "following changes no coverage (a mirror that shows nothing stays recorded)");
    expect(!same(plain.depth, two.depth) && !same(plain.albedo, two.albedo), "mirrorBounces = 2 differs from the plain pass");
    auto integ = make();
    integ->RenderFeatures(*b.scene, 0, 3, &cut, 2);
    integ->RenderFeatures(*b.scene, 3, 5, &cut, 2);
    expect(same(two, cut), "RenderFeatures(0, 8) equals (0, 3) then (3, 5) with mirrorBounces = 2, bit for bit");
    if (dump0 && dump2) {
        expect(equals_image(dump0, plain, W, H), "the default buffers equal the C-ABI image of the plain pass");
        expect(equals_image(dump2, two, W, H), "mirrorBounces = 2 equals the C-ABI image with max_bounces = 2");
    }
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    try {
        const int rc = mode == "gpu" ? run_gpu(argc > 3 ? argv[2] : nullptr, argc > 3 ? argv[3] : nullptr) : run_cpu();
        std::printf("%s: %d failure(s)\n", mode.c_str(), failures);
        return rc;
    } catch (const std::exception& e) {
        std::printf("FAIL uncaught: %s\n", e.what());
        return 2;
    }
}
