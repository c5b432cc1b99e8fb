// aov_test.cpp — SamplerIntegrator::RenderFeatures (include/pbr/pbr.h): feature buffers through the C++
// host API.
//
//   aov_test cpu          no GPU needed: bad parameters and a custom sampler are refused; without a device
//                         the call fails loudly
//   aov_test gpu [file]   RenderFeatures(0, 8) equals RenderFeatures(0, 3) followed by RenderFeatures(3, 5),
//                         bit for bit; SetTiles leaves the pixels outside the tiles 0; with `file` (40·30·8
//                         float32: the C-ABI image of the same frame, written by tests/test_host_aov.py) the
//                         buffers equal it
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

// One matte ball of radius 1.5 at the origin under a point light, seen from z = 5 (tests/cpp_adaptive's
// scene; tests/test_host_aov.py builds the same one through the Python layer).
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

template <class Fn> bool throws_invalid(Fn fn) {
    try {
        fn();
    } catch (const std::invalid_argument& e) {
        std::printf("     (%s)\n", e.what());
        return true;
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
    build_ball(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    FeatureBuffers out;
    auto halton = [&] { return std::make_shared<WhittedIntegrator>(5, b.cam, std::make_shared<HaltonSampler>(8, bounds), bounds, &fb); };
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, 0, 0, &out); }), "nSamples below 1 is refused");
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, -1, 2, &out); }), "a negative firstSample is refused");
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, 0, 2, nullptr); }), "out == nullptr is refused");
    expect(throws_invalid([&] { halton()->RenderFeatures(*b.scene, 3, 2, &out); }), "a pass that continues nothing is refused");
    bool threw = false;
    try {
        auto integ = std::make_shared<WhittedIntegrator>(5, b.cam, std::make_shared<ForwardingHalton>(8, bounds), bounds, &fb);
        integ->RenderFeatures(*b.scene, 0, 2, &out);
    } catch (const std::invalid_argument& e) {
        threw = std::string(e.what()).find("custom sampler") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderFeatures refuses an integrator built on a custom (table) sampler");
    threw = false;
    try {
        halton()->RenderFeatures(*b.scene, 0, 2, &out);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("pbr_hip_create") != std::string::npos;
        std::printf("     (%s)\n", e.what());
    }
    expect(threw, "RenderFeatures without a GPU throws from pbr_hip_create");
    return failures ? 1 : 0;
}

int run_gpu(const char* dump) {
    const int W = 40, H = 30, spp = 8;
    const Bounds2i bounds(Point2i(0, 0), Point2i(W, H));
    Built b;
    build_ball(b, W, H);
    FrameBuffer fb;
    fb.InitBuffer(W, H, 4);
    auto make = [&] { return std::make_shared<PathIntegrator>(8, b.cam, std::make_shared<HaltonSampler>(spp, bounds), bounds, 0.8f, "uniform", &fb); };
    FeatureBuffers one, part, two;
    make()->RenderFeatures(*b.scene, 0, 8, &one);
    auto integ = make();
    integ->RenderFeatures(*b.scene, 0, 3, &part);
    expect(throws_invalid([&] { integ->RenderFeatures(*b.scene, 4, 2, &two); }), "a gap in the samples is refused");
    integ->RenderFeatures(*b.scene, 3, 5, &two);
    expect(one.width == W && one.height == H && one.albedo.size() == (size_t)W * H * 3 && one.depth.size() == (size_t)W * H,
           "the buffers cover the pixel bounds");
    expect(same(one, two), "RenderFeatures(0, 8) equals RenderFeatures(0, 3) then RenderFeatures(3, 5), bit for bit");
    expect(!same(one.depth, part.depth) || !same(one.normal, part.normal), "... and differs from the image after 3 samples");
    // the ball covers the centre and not the corners
    const size_t centre = (size_t)(H / 2) * W + W / 2;
    expect(one.coverage[centre] == 1.f && one.albedo[3 * centre] == 0.5f && std::fabs(one.albedo[3 * centre + 1] - 0.6f) < 1e-6f &&
               std::fabs(one.albedo[3 * centre + 2] - 0.7f) < 1e-6f && std::fabs(one.depth[centre] - 3.5f) < 0.05f &&
               one.normal[3 * centre + 2] > 0.9f,
           "the centre pixel sees the ball: its Kd, a distance near 3.5, a normal towards the camera");
    expect(one.coverage[0] == 0.f && one.depth[0] == 0.f && one.albedo[0] == 0.f, "a corner pixel sees nothing");
    // tiles: the pixels outside are left 0, those inside are the frame's
    const std::vector<Bounds2i> tiles = {Bounds2i(Point2i(17, 12), Point2i(22, 15)), Bounds2i(Point2i(3, 20), Point2i(10, 22))};
    auto tiled = make();
    tiled->SetTiles(tiles);
    FeatureBuffers t;
    tiled->RenderFeatures(*b.scene, 0, 8, &t);
    bool inside = true, outside = true;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool in = false;
            for (const Bounds2i& tb : tiles) in = in || (x >= tb.pMin.x && x < tb.pMax.x && y >= tb.pMin.y && y < tb.pMax.y);
            const size_t p = (size_t)y * W + x;
            if (in) {
                inside = inside && std::memcmp(&t.albedo[3 * p], &one.albedo[3 * p], 12) == 0 &&
                         std::memcmp(&t.normal[3 * p], &one.normal[3 * p], 12) == 0 && std::memcmp(&t.depth[p], &one.depth[p], 4) == 0 &&
                         std::memcmp(&t.coverage[p], &one.coverage[p], 4) == 0;
            } else {
                outside = outside && t.albedo[3 * p] == 0.f && t.normal[3 * p + 2] == 0.f && t.depth[p] == 0.f && t.coverage[p] == 0.f;
            }
        }
    expect(inside, "SetTiles: the tiles' pixels are the whole frame's");
    expect(outside, "SetTiles: the pixels outside the tiles are 0");
    if (dump) {   // the C-ABI image of the same frame: [pixel][8] float32
        std::vector<float> img((size_t)W * H * 8);
        FILE* f = std::fopen(dump, "rb");
        const size_t got = f ? std::fread(img.data(), sizeof(float), img.size(), f) : 0;
        if (f) std::fclose(f);
        expect(got == img.size(), std::string("read ") + dump);
        bool eq = got == img.size();
        for (size_t p = 0; eq && p < (size_t)W * H; ++p)
            eq = std::memcmp(&img[8 * p], &one.albedo[3 * p], 12) == 0 && std::memcmp(&img[8 * p + 3], &one.coverage[p], 4) == 0 &&
                 std::memcmp(&img[8 * p + 4], &one.normal[3 * p], 12) == 0 && std::memcmp(&img[8 * p + 7], &one.depth[p], 4) == 0;
        expect(eq, "the buffers equal the C-ABI image of the same frame");
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
