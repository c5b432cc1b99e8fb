// spatial_test.cpp — SamplerIntegrator::Denoise with the spatial variance estimate (DenoiseParams::
// spatialMinCount, include/pbr/pbr.h): an image of one sample per pixel through the C++ host API.
//
//   spatial_test cpu          no GPU needed: spatialMinCount and spatialRadius out of range and missing passes
//                             are refused before any device call
//   spatial_test gpu [file]   after RenderSamples(0, 1) and RenderFeatures(0, 1) on the ball scene the default
//                             parameters still throw; with spatialMinCount = 4 Denoise fills the FrameBuffer,
//                             twice with the same bits; with `file` (40·30·3 float32 then 40·30·4 bytes: the
//                             C-ABI result of the same frame, rows top-down, written by
//                             tests/test_host_spatial_variance.py) the FrameBuffer equals it, flipped
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

// One matte ball of radius 1.5 at the origin under a point light, seen from z = 5 (tests/cpp_aov's scene;
// tests/test_host_denoise.py builds the same one through the Python layer).
void build_ball(Built& b, int W, int H) {
    std::vector<std::shared_ptr<Primitive>> prims;
    auto matte = std::make_shared<MatteMaterial>(rgbTex(0.5f, 0.6f, 0.7f), fTex(0.f), nullptr);
    const Transform* o2w = keep(b, Transform());
    const Transform* w2o = keep(b, Inverse(*o2w));
    prims.push_back(std::make_shared<GeometricPrimitive>(std::make_shared<Sphere>(o2w, w2o, false, 1.5f), matte, nullptr,
                                                         MediumInterface()));
    std::vector<std::shared_ptr<Light>> lights;
    lights.push_back(std::make_shared<PointLight>(Translate(Vector3f(0.f, 4.f, 4.f)), MediumInterface(), Spectrum(20.f)));
    b.scene = std::make_unique<Scene>(std::make_shared<BVHAccel>(prims, 1), lights);
    Transform lookat = LookAt(Point3f(0.f, 0.f, 5.f), Point3f(0.f, 0.f, 0.f), Vector3f(0.f, 1.f, 0.f));
    b.cam = std::shared_ptr<Camera>(CreatePerspectiveCamera(W, H, Inverse(lookat), nullptr));
}

template <class Fn> bool throws_invalid(Fn fn, const char* needle = nullptr) {
    try {
        fn();
    } catch (const std::invalid_argument& e) {
        std::printf("     (%s)\n", e.what());
        return !needle || std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

DenoiseParams spatial(int minCount, int radius = 1) {
    DenoiseParams p;
    p.spatialMinCount = minCount;
    p.spatialRadius = radius;
    return p;
}

int run_cpu() {
    const int W = 32, H = 24;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_ball(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    auto make = [&] { return std::make_shared<PathIntegrator>(8, b.cam, std::make_shared<HaltonSampler>(8, bounds), bounds, 0.8f, "uniform", &fb); };
    expect(DenoiseParams().spatialMinCount == 0, "the estimate is off by default");
    expect(throws_invalid([&] { make()->Denoise(spatial(1)); }, "spatialMinCount"), "spatialMinCount 1 is refused");
    expect(throws_invalid([&] { make()->Denoise(spatial(65)); }, "spatialMinCount"), "spatialMinCount 65 is refused");
    expect(throws_invalid([&] { make()->Denoise(spatial(-4)); }, "spatialMinCount"), "a negative spatialMinCount is refused");
    expect(throws_invalid([&] { make()->Denoise(spatial(4, 0)); }, "spatialRadius"), "spatialRadius 0 is refused");
    expect(throws_invalid([&] { make()->Denoise(spatial(4, 4)); }, "spatialRadius"), "spatialRadius 4 is refused");
    expect(throws_invalid([&] { make()->Denoise(spatial(4)); }, "needs 1"), "Denoise before any RenderSamples pass is refused");
    expect(throws_invalid([&] { make()->Denoise(); }, "needs 2"), "... and by default with the message it had");
    return failures ? 1 : 0;
}

std::vector<float> floats(FrameBuffer& fb, int W, int H) {
    std::vector<float> v((size_t)W * H * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < 3; ++c) v[((size_t)y * W + x) * 3 + c] = fb.getFCbuffer()[((size_t)y * W + x) * fb.channals + c];
    return v;
}
bool same(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int run_gpu(const char* dump) {
    const int W = 40, H = 30, spp = 8;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_ball(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    auto integ = std::make_shared<PathIntegrator>(8, b.cam, std::make_shared<HaltonSampler>(spp, bounds), bounds, 0.8f, "uniform", &fb);
    FeatureBuffers feats;
    integ->RenderSamples(*b.scene, 0, 1);
    expect(throws_invalid([&] { integ->Denoise(spatial(4)); }, "RenderFeatures"), "Denoise without RenderFeatures is refused");
    integ->RenderFeatures(*b.scene, 0, 1, &feats);
    const std::vector<float> noisy = floats(fb, W, H);
    expect(throws_invalid([&] { integ->Denoise(); }, "needs 2"), "the default parameters still refuse one sample");
    expect(same(floats(fb, W, H), noisy), "... and leave the FrameBuffer");
    integ->Denoise(spatial(4));
    const std::vector<float> once = floats(fb, W, H);
    const std::vector<unsigned char> once8(fb.getUCbuffer(), fb.getUCbuffer() + (size_t)W * H * fb.channals);
    bool finite = true, light = false;
    for (float v : once) { finite = finite && std::isfinite(v); light = light || v > 0.f; }
    expect(finite && light, "with spatialMinCount = 4 Denoise fills the FrameBuffer with a finite image");
    expect(!same(once, noisy), "... which is not the one-sample image");
    integ->Denoise(spatial(4));
    expect(same(floats(fb, W, H), once), "a second Denoise gives the same bits (the sums are left as they are)");
    integ->Denoise(spatial(4, 3));
    expect(!same(floats(fb, W, H), once), "radius 3 differs from radius 1");
    if (dump) {   // the C-ABI result of the same frame, rows top-down: [pixel][3] float32, then [pixel][4] bytes
        std::vector<float> rgb((size_t)W * H * 3);
        std::vector<unsigned char> rgba((size_t)W * H * 4);
        FILE* f = std::fopen(dump, "rb");
        const size_t got = f ? std::fread(rgb.data(), sizeof(float), rgb.size(), f) : 0;
        const size_t got8 = f ? std::fread(rgba.data(), 1, rgba.size(), f) : 0;
        if (f) std::fclose(f);
        expect(got == rgb.size() && got8 == rgba.size(), std::string("read ") + dump);
        bool eq = got == rgb.size() && got8 == rgba.size(), eq8 = eq;
        for (int y = 0; eq && y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x, q = (size_t)(H - y - 1) * W + x;   // (the FrameBuffer is flipped)
                eq = eq && std::memcmp(&rgb[3 * p], &once[3 * q], 12) == 0;
                eq8 = eq8 && std::memcmp(&rgba[4 * p], &once8[q * fb.channals], 4) == 0;
            }
        expect(eq, "the FrameBuffer's floats equal the C-ABI result of the same frame, flipped");
        expect(eq8, "... and its bytes");
    }
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    try {
        const int rc = mode == "gpu" ? run_gpu(argc > 2 ? argv[2] : nullptr) : run_cpu();
        std::printf("%s: %d failure(s)\n", mode.c_str(), failures);
        return rc;
    } catch (const std::exception& e) {
        std::printf("FAIL uncaught: %s\n", e.what());
        return 2;
    }
}
