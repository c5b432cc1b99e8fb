// adaptive_test.cpp — SamplerIntegrator::RenderAdaptive (include/pbr/pbr.h): adaptive sampling through
// the C++ host API.
//
//   adaptive_test cpu   no GPU needed: bad parameters and a custom sampler are refused; without a device
//                       the call fails loudly
//   adaptive_test gpu   RenderAdaptive fills the FrameBuffer; a huge tolerance leaves the bytes of
//                       RenderSamples(0, minSamples); a tolerance of 0 over a tile in which every pixel
//                       has variance leaves the bytes of Render
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

// One matte ball of radius 1.5 at the origin under a point light, seen from z = 5 (90° vertical field
// of view): it covers the middle of the raster — about 4.7 pixels around the centre at 40×30 — where
// the shading varies over every pixel; the background is black, so its pixels have no variance.
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

// a GlobalSampler the device cannot compute: its values go over as a whole frame's table
class ForwardingHalton : public GlobalSampler {
  public:
    ForwardingHalton(int spp, const Bounds2i& b) : GlobalSampler(spp), inner(spp, b) {}
    void StartPixel(const Point2i& p) override {
        inner.StartPixel(p);
        GlobalSampler::StartPixel(p);
    }
    int64_t GetIndexForSample(int64_t sampleNum) const override { return inner.GetIndexForSample(sampleNum); }
    float SampleDimension(int64_t index, int dimension) const override { return inner.SampleDimension(index, dimension); }
    std::unique_ptr<Sampler> Clone(int) override { return std::unique_ptr<Sampler>(new ForwardingHalton(*this)); }

  private:
    HaltonSampler inner;
};

std::shared_ptr<SamplerIntegrator> make_integrator(int itype, const Built& b, std::shared_ptr<Sampler> smp, const Bounds2i& bounds,
                                                   FrameBuffer* fb) {
    if (itype == 0) return std::make_shared<WhittedIntegrator>(5, b.cam, smp, bounds, fb);
    return std::make_shared<PathIntegrator>(8, b.cam, smp, bounds, 0.8f, "uniform", fb);
}

template <class Fn> bool throws_invalid(Fn fn) {
    try {
        fn();
    } catch (const std::invalid_argument& e) {
        std::printf("     (%s)\n", e.what());
        return true;
    }
    return false;
}

int run_cpu() {
    const int W = 32, H = 24;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_ball(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    auto halton = [&] { return make_integrator(0, b, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb); };
    expect(throws_invalid([&] { halton()->RenderAdaptive(*b.scene, 1, 2, 0.05f, 1e-3f); }), "minSamples below 2 is refused");
    expect(throws_invalid([&] { halton()->RenderAdaptive(*b.scene, 9, 2, 0.05f, 1e-3f); }), "minSamples above the budget is refused");
    expect(throws_invalid([&] { halton()->RenderAdaptive(*b.scene, 2, 0, 0.05f, 1e-3f); }), "samplesPerRound below 1 is refused");
    expect(throws_invalid([&] { halton()->RenderAdaptive(*b.scene, 2, 2, -1.f, 1e-3f); }), "a negative tolerance is refused");
    expect(throws_invalid([&] { halton()->RenderAdaptive(*b.scene, 2, 2, 0.05f, std::nanf("")); }),
           "a NaN floor is refused");
    bool threw = false;
    try {
        auto integ = make_integrator(0, b, std::make_shared<ForwardingHalton>(8, bounds), bounds, &fb);
        integ->RenderAdaptive(*b.scene, 2, 2, 0.05f, 1e-3f);
    } catch (const std::invalid_argument& e) {
        threw = std::string(e.what()).find("custom sampler") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderAdaptive refuses an integrator built on a custom (table) sampler");
    threw = false;
    try {
        halton()->RenderAdaptive(*b.scene, 2, 2, 0.05f, 1e-3f);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("pbr_hip_create") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderAdaptive without a GPU throws from pbr_hip_create");
    return failures ? 1 : 0;
}

int run_gpu() {
    const int W = 40, H = 30, spp = 8, minS = 2;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    const size_t nb = (size_t)W * H * 4;
    for (int itype = 0; itype < 2; ++itype) {
        const std::string name = itype ? "Path" : "Whitted";
        Built b;
        build_ball(b, W, H);
        auto smp = [&] { return std::make_shared<HaltonSampler>(spp, bounds); };
        // a huge tolerance: every pixel stops at minSamples
        FrameBuffer two, ada;
        two.InitBuffer(W, H, 4);
        ada.InitBuffer(W, H, 4);
        make_integrator(itype, b, smp(), bounds, &two)->RenderSamples(*b.scene, 0, minS);
        auto integ = make_integrator(itype, b, smp(), bounds, &ada);
        std::vector<int> counts = integ->RenderAdaptive(*b.scene, minS, 2, 1e30f, 1e-3f);
        bool all = counts.size() == (size_t)W * H;
        for (int c : counts) all = all && c == minS;
        expect(all, name + ": a huge tolerance stops every pixel at minSamples");
        expect(std::memcmp(two.getUCbuffer(), ada.getUCbuffer(), nb) == 0 &&
                   std::memcmp(two.getFCbuffer(), ada.getFCbuffer(), nb * sizeof(float)) == 0,
               name + ": ... and leaves the FrameBuffer of RenderSamples(0, minSamples), bytes and floats");
        expect(throws_invalid([&] { integ->RenderSamples(*b.scene, minS, 2); }), name + ": a RenderSamples pass cannot continue it");
        // a working tolerance: the black background stops at once, the ball goes on
        counts = integ->RenderAdaptive(*b.scene, minS, 2, 0.01f, 1e-3f);
        int lo = spp, hi = 0;
        for (int c : counts) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
        expect(counts[0] == minS && lo == minS && hi > minS && hi <= spp && integ->LastStats().samples < (uint64_t)W * H * spp,
               name + ": at 1% the background stops at minSamples, the ball does not");
        // tolerance 0 over a tile inside the ball: every pixel has variance, so all reach the budget
        const std::vector<Bounds2i> tile = {Bounds2i(Point2i(18, 13), Point2i(22, 17))};
        FrameBuffer ref, zero;
        ref.InitBuffer(W, H, 4);
        zero.InitBuffer(W, H, 4);
        double t = 0;
        auto full = make_integrator(itype, b, smp(), bounds, &ref);
        full->SetTiles(tile);
        full->Render(*b.scene, t);
        auto az = make_integrator(itype, b, smp(), bounds, &zero);
        az->SetTiles(tile);
        counts = az->RenderAdaptive(*b.scene, minS, 3, 0.f, 1e-3f);
        all = counts.size() == 16;
        for (int c : counts) all = all && c == spp;
        expect(all, name + ": tolerance 0 takes every pixel of a tile inside the ball to the budget");
        expect(std::memcmp(ref.getUCbuffer(), zero.getUCbuffer(), nb) == 0 &&
                   std::memcmp(ref.getFCbuffer(), zero.getFCbuffer(), nb * sizeof(float)) == 0,
               name + ": ... and leaves Render's FrameBuffer, bytes and floats");
    }
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    try {
        const int rc = mode == "gpu" ? run_gpu() : run_cpu();
        std::printf("%s: %d failure(s)\n", mode.c_str(), failures);
        return rc;
    } catch (const std::exception& e) {
        std::printf("FAIL uncaught: %s\n", e.what());
        return 2;
    }
}
