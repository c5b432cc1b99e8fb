// progressive_test.cpp — SamplerIntegrator::RenderSamples (include/pbr/pbr.h): a frame's samples in
// resumable passes over sums kept on the integrator's device.
//
//   progressive_test cpu   no GPU needed: a custom sampler is refused; without a device the call fails loudly
//   progressive_test gpu   RenderSamples(0, 3) then RenderSamples(3, 5) leaves the FrameBuffer bytes and
//                          float buffer of Render at 8 spp (Whitted, Path); a pass that does not continue
//                          the samples done is refused
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

// Two matte spheres under a point light; `floor`: over a matte floor (the Path scene).
void build_spheres(Built& b, int W, int H, bool floor) {
    std::vector<std::shared_ptr<Primitive>> prims;
    auto matte = std::make_shared<MatteMaterial>(rgbTex(0.5f, 0.5f, 0.5f), fTex(0.f), nullptr);
    const Vector3f centres[2] = {Vector3f(-1.f, 0.f, 0.f), Vector3f(1.2f, 0.f, -1.f)};
    for (const Vector3f& c : centres) {
        const Transform* o2w = keep(b, Translate(c));
        const Transform* w2o = keep(b, Inverse(*o2w));
        prims.push_back(std::make_shared<GeometricPrimitive>(std::make_shared<Sphere>(o2w, w2o, false, 1.f), matte, nullptr,
                                                             MediumInterface()));
    }
    if (floor) {
        auto floorMat = std::make_shared<MatteMaterial>(rgbTex(0.6f, 0.7f, 0.6f), fTex(0.f), nullptr);
        const Transform* id = keep(b, Transform());
        const Point3f fp[4] = {Point3f(-5, -1, -5), Point3f(5, -1, -5), Point3f(5, -1, 5), Point3f(-5, -1, 5)};
        const int fi[6] = {0, 2, 1, 0, 3, 2};
        for (auto& s : CreateTriangleMesh(id, id, false, 2, fi, 4, fp, nullptr, nullptr, nullptr))
            prims.push_back(std::make_shared<GeometricPrimitive>(s, floorMat, nullptr, MediumInterface()));
    }
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

int run_cpu() {
    const int W = 32, H = 24;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_spheres(b, W, H, false);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    bool threw = false;
    try {
        auto integ = make_integrator(0, b, std::make_shared<ForwardingHalton>(8, bounds), bounds, &fb);
        integ->RenderSamples(*b.scene, 0, 4);
    } catch (const std::invalid_argument& e) {
        threw = std::string(e.what()).find("custom sampler") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderSamples refuses an integrator built on a custom (table) sampler");
    threw = false;
    try {
        auto integ = make_integrator(0, b, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb);
        integ->RenderSamples(*b.scene, 0, 0);
    } catch (const std::invalid_argument&) { threw = true; }
    expect(threw, "RenderSamples refuses an empty pass");
    threw = false;
    try {
        auto integ = make_integrator(0, b, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb);
        integ->RenderSamples(*b.scene, 3, 5);
    } catch (const std::invalid_argument&) { threw = true; }
    expect(threw, "RenderSamples refuses a first pass that does not start at sample 0");
    threw = false;
    try {
        auto integ = make_integrator(0, b, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb);
        integ->RenderSamples(*b.scene, 0, 4);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("pbr_hip_create") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderSamples without a GPU throws from pbr_hip_create");
    return failures ? 1 : 0;
}

int run_gpu() {
    const int W = 40, H = 30, spp = 8;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    const size_t nb = (size_t)W * H * 4;
    for (int itype = 0; itype < 2; ++itype) {
        const std::string name = itype ? "Path" : "Whitted";
        Built b;
        build_spheres(b, W, H, itype == 1);
        FrameBuffer ref, prog;
        ref.InitBuffer(W, H, 4);
        prog.InitBuffer(W, H, 4);
        double t = 0;
        make_integrator(itype, b, std::make_shared<HaltonSampler>(spp, bounds), bounds, &ref)->Render(*b.scene, t);
        auto integ = make_integrator(itype, b, std::make_shared<HaltonSampler>(spp, bounds), bounds, &prog);
        integ->RenderSamples(*b.scene, 0, 3);
        expect(integ->SamplesDone() == 3 && std::memcmp(ref.getFCbuffer(), prog.getFCbuffer(), nb * sizeof(float)) != 0,
               name + ": after 3 of 8 samples the image is not yet the frame's");
        bool threw = false;
        try {
            integ->RenderSamples(*b.scene, 4, 4);
        } catch (const std::invalid_argument&) { threw = true; }
        expect(threw && integ->SamplesDone() == 3, name + ": a pass that skips a sample is refused");
        integ->RenderSamples(*b.scene, 3, 5);
        expect(integ->SamplesDone() == 8, name + ": 8 samples done");
        expect(std::memcmp(ref.getUCbuffer(), prog.getUCbuffer(), nb) == 0,
               name + ": RenderSamples(0, 3) + RenderSamples(3, 5) leaves Render's FrameBuffer bytes");
        expect(std::memcmp(ref.getFCbuffer(), prog.getFCbuffer(), nb * sizeof(float)) == 0,
               name + ": ... and its float buffer, bit for bit");
        threw = false;
        try {
            integ->RenderSamples(*b.scene, 8, 1);
        } catch (const std::runtime_error&) { threw = true; }
        expect(threw, name + ": a pass beyond the sampler's samplesPerPixel is refused");
        // a new image from sample 0 reuses the device buffers
        integ->RenderSamples(*b.scene, 0, 8);
        expect(std::memcmp(ref.getFCbuffer(), prog.getFCbuffer(), nb * sizeof(float)) == 0,
               name + ": one pass of all 8 samples is Render's frame");
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
