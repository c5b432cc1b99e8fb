/*
 * pbr_hip.h — C-ABI drop-in boundary for the MI355X render path.
 *
 * The reference (G0T-cha/PysicalBasedRaytracer) has no FFI: its hot path is reached through the
 * C++ virtual `Integrator::Render(const Scene&, double&)` (Integrator/Integrator.h:14) after the
 * scene has been assembled from `GeometricPrimitive`s (Core/Primitive.h:30-33), a `BVHAccel`
 * (Accelerator/BVHAccel.h:19-21), lights (Light/Light.h:50-61), a `HaltonSampler`
 * (Sampler/Halton.h:18) and a `PerspectiveCamera` (Camera/Perspective.cpp:84-104).
 * The C++ host mirror in include/pbr/ keeps those class names and constructors; underneath, every
 * one of them flattens into the POD descriptors below and crosses into the HIP runtime through the
 * five `pbr_hip_*` entry points.  Nothing here uses torch or STL types: plain pointers and sizes.
 *
 * Entry point ↔ reference interface it replaces:
 *   pbr_hip_create        — (none; the reference has one implicit CPU "device")
 *   pbr_hip_upload_scene  — Scene::Scene (Core/Scene.cpp:7-17) + BVHAccel::BVHAccel
 *                           (Accelerator/BVHAccel.cpp:57-87) + TriangleMesh ctor (Shape/Triangle.cpp:12-44)
 *                           + HaltonSampler ctor (Sampler/Halton.cpp:30-58)
 *   pbr_hip_render        — SamplerIntegrator::Render (Integrator/Integrator.cpp:280-356), which
 *                           drives {Whitted,Path,VolPath}Integrator::Li per sample
 *   pbr_hip_render_passes — (none; the reference renders whole frames): that Render's sample loop in
 *                           resumable passes over a carried per-pixel sum (progressive rendering)
 *   pbr_hip_render_adaptive — (none): those passes with a per-pixel stopping rule (adaptive sampling;
 *                           pbr_hip_adaptive_select and pbr_hip_render_passes_list are its two steps)
 *   pbr_hip_render_aov    — (none): per-pixel albedo, coverage, normal and depth of the first surface the
 *                           same camera samples see, in the same resumable passes (feature buffers)
 *   pbr_hip_render_aov_mirrors — (none): that pass with mirror bounces followed, so that a mirror records the
 *                           surface it reflects at the unfolded distance (pbr_hip_mirror_step_host: one
 *                           step on the CPU)
 *   pbr_hip_denoise       — (none): an edge-avoiding à-trous filter over those sums and feature buffers
 *   pbr_hip_denoise_sv    — (none): that filter with a spatial variance estimate before its first level, so
 *                           that pixels with one sample are filtered (pbr_hip_spatial_variance_host: the
 *                           estimate on the CPU)
 *   pbr_hip_temporal      — (none): the previous frame's sums reprojected into this frame's (temporal
 *                           accumulation; pbr_hip_camera_matrices gives it a camera's matrices)
 *   pbr_hip_destroy      — scene/integrator destructors
 *   pbr_hip_last_error    — (none; the reference fails silently)
 *   pbr_hip_sync          — (none; the reference's Render returns when the frame is done): waits
 *                           for asynchronous frames and reports a deferred failure
 *
 * Errors: every call returns 0 on success, a negative PBR_E_* code otherwise; the message is
 * kept per context and returned by pbr_hip_last_error.  Calls on one context are not thread-safe;
 * different contexts (one per device) are independent.
 *
 * Unbounded walks: the reference follows chains of material-less surfaces (medium boundaries)
 * without limit (WhittedIntegrator.cpp:26-28, PathIntegrator.cpp:70-75, Light.cpp:31-47).  The
 * device follows them too, up to safety bounds far beyond any sane scene — 1024 crossings in one
 * Whitted Li or Path/VolPath path, 256 interfaces on one transmittance walk — and a frame in which
 * a walk reaches a bound fails with PBR_E_UNSUPPORTED (synchronous renders: that call;
 * asynchronous ones: the next pbr_hip_render or pbr_hip_sync on the context) instead of returning
 * a truncated image.  BVH traversal keeps the reference's 64-entry stack (BVHAccel.cpp:293): an
 * upload whose tree could overflow it (or the 1.5-entries-per-level need of the two-level node walk)
 * fails with PBR_E_UNSUPPORTED.
 */
#ifndef PBR_HIP_H
#define PBR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBR_HIP_ABI_VERSION 5

/* ---- status codes ---- */
enum {
    PBR_OK = 0,
    PBR_E_INVALID = -1,   /* bad argument / descriptor */
    PBR_E_HIP = -2,       /* a HIP runtime call failed */
    PBR_E_NOSCENE = -3,   /* render before upload */
    PBR_E_UNSUPPORTED = -4,
    PBR_E_NODEVICE = -5
};

/* ---- enums mirroring the reference's class families ---- */
enum pbr_shape_type { PBR_SHAPE_TRIANGLE_MESH = 0, PBR_SHAPE_SPHERE = 1 };
enum pbr_material_type {
    PBR_MAT_NONE = 0,     /* GeometricPrimitive with material == nullptr (medium boundary) */
    PBR_MAT_MATTE = 1,    /* Material/MatteMaterial.cpp:13-28 */
    PBR_MAT_MIRROR = 2,   /* Material/Mirror.cpp:5-15 */
    PBR_MAT_GLASS = 3,    /* Material/GlassMaterial.cpp:9-57 */
    PBR_MAT_METAL = 4,    /* Material/MetalMaterial.cpp:25-43 */
    PBR_MAT_PLASTIC = 5   /* Material/PlasticMaterial.cpp:8-30 */
};
enum pbr_light_type {
    PBR_LIGHT_POINT = 0,        /* Light/PointLight.cpp */
    PBR_LIGHT_DIFFUSE_AREA = 1, /* Light/DiffuseLight.cpp */
    PBR_LIGHT_SKYBOX = 2,       /* Light/SkyBoxLight.cpp */
    PBR_LIGHT_INFINITE_AREA = 3 /* Light/InfiniteAreaLight.cpp: light_to_world, Le = the `power`
                                 * scale, n_samples, env_* = the image as stbi_loadf returned it
                                 * (NULL → a 1x1 map of Le); worldRadius from the scene bounds.
                                 * A caller holding only a built light's map — Lmap's level 0
                                 * (InfiniteAreaLight.h:33: powers of two, L already applied) —
                                 * passes those texels with Le = (1, 1, 1): 1·x is x, a power-of-two
                                 * image is not resampled (MIPMap.h:96), so the upload rebuilds the
                                 * same pyramid, Distribution2D and Power() */
};
enum pbr_integrator_type {
    PBR_INTEGRATOR_WHITTED = 0, /* Integrator/WhittedIntegrator.cpp:11-65 */
    PBR_INTEGRATOR_PATH = 1,    /* Integrator/PathIntegrator.cpp:32-110 */
    PBR_INTEGRATOR_VOLPATH = 2  /* Integrator/VolPathIntegrator.cpp:21-107 */
};
/* HALTON: Sampler/Halton.cpp; SOBOL: pbrt-v3's SobolSampler over the reference's SobolMatrices32;
 * TABLE: values supplied by the caller — a host sampler the device cannot compute, e.g. a custom
 * GlobalSampler subclass (Sampler/Sampler.h:62-82): see pbr_render_desc::sample_table. */
enum pbr_sampler_type { PBR_SAMPLER_HALTON = 0, PBR_SAMPLER_SOBOL = 1, PBR_SAMPLER_TABLE = 2 };
enum pbr_light_strategy { PBR_LIGHTS_UNIFORM = 0, PBR_LIGHTS_POWER = 1 };
/* BVHAccel::SplitMethod (Accelerator/BVHAccel.h:18); HLBVH falls through to SAH (BVHAccel.cpp:135-160). */
enum pbr_split_method { PBR_SPLIT_SAH = 0, PBR_SPLIT_HLBVH = 1, PBR_SPLIT_MIDDLE = 2, PBR_SPLIT_EQUAL_COUNTS = 3 };

/* A reference Transform holds both m and mInv (Core/Transform.h:49-60); so do we. Row-major. */
typedef struct pbr_transform {
    float m[16];
    float m_inv[16];
} pbr_transform;

/* One Shape family instance. Primitives are enumerated in shape order, triangles in index order:
 * this is the `prims` vector order the reference hands to BVHAccel (Main/main.cpp:279-282). */
typedef struct pbr_shape_desc {
    int type;                   /* pbr_shape_type */
    pbr_transform object_to_world;
    int reverse_orientation;
    /* triangle mesh (Shape/Triangle.h:11-24) */
    int n_triangles;
    int n_vertices;
    const int32_t* indices;     /* 3*n_triangles */
    const float* P;             /* 3*n_vertices, object space */
    const float* N;             /* optional 3*n_vertices per-vertex normals (object space), or NULL */
    const float* UV;            /* optional 2*n_vertices, or NULL (default (0,0),(1,0),(1,1)) */
    /* sphere (Shape/Sphere.h) */
    float radius;
    /* GeometricPrimitive fields (Core/Primitive.h:30-33) */
    int material;               /* index into materials, -1 = nullptr */
    int area_light_first;       /* triangle t carries lights[area_light_first + t]; -1 = none */
    int medium_inside;          /* MediumInterface, -1 = nullptr */
    int medium_outside;
} pbr_shape_desc;

/* ImageTexture<RGBSpectrum, Spectrum> / <float, float> (Texture/ImageTexture.h:43-91,
 * ImageTexture.cpp:13-92) with a UVMapping2D (Texture/Texture.h:16-27).  The reference's ray
 * differentials are zero (dudx = dvdx = 0, F5), so both MIPMap filters — trilinear (MIPMap.h:193-211)
 * and EWA (:227-247) — reduce to the bilinear level-0 lookup triangle(0, st) (:240-252); the pyramid
 * above level 0 is never read.  Level 0 is the image resampled to powers of two with the texture's
 * wrap mode (MIPMap.h:86-150). */
enum pbr_image_wrap { PBR_WRAP_REPEAT = 0, PBR_WRAP_BLACK = 1, PBR_WRAP_CLAMP = 2 };   /* ImageWrap, MIPMap.h:21 */
typedef struct pbr_texture_desc {
    int is_float;               /* 1: ImageTexture<float, float> (convertIn: scale * y()), 0: RGB */
    int width, height, components;
    const float* data;          /* as loadImage's stbi_loadf returns it (flip-on-load set); NULL →
                                 * the 1x1 grey 0.5 image GetTexture substitutes (ImageTexture.cpp:60-66) */
    float scale;
    int gamma;                  /* convertIn applies InverseGammaCorrect (Core/PBR.h:126-129) */
    int wrap;                   /* pbr_image_wrap */
    int trilinear;              /* doTrilinear (no effect, see above) */
    float max_aniso;            /* maxAniso (no effect, see above) */
    float su, sv, du, dv;       /* UVMapping2D(su, sv, du, dv): st = (su·u + du, sv·v + dv) */
    int level0;                 /* 1: `data` is already the MIPMap's level 0 — what a built ImageTexture
                                 * holds (ImageTexture.h:88, MIPMap.h:150-153): width and height powers
                                 * of two, convertIn applied, `components` = 3 (RGB) or 1 (float
                                 * textures); used as is (scale and gamma ignored) */
} pbr_texture_desc;

/* Material parameter slots that may hold an image texture instead of the constant below
 * (pbr_material_desc.tex[slot] = index into pbr_scene_desc.textures + 1; 0 = the constant, so a
 * zero-initialised descriptor has no textures).  RGB slots need an RGB texture, scalar slots a
 * float one. */
enum pbr_texture_slot {
    PBR_TEX_KD = 0,             /* matte / plastic Kd (RGB) */
    PBR_TEX_KS = 1,             /* plastic Ks (RGB) */
    PBR_TEX_KR = 2,             /* mirror / glass Kr (RGB) */
    PBR_TEX_KT = 3,             /* glass Kt (RGB) */
    PBR_TEX_SIGMA = 4,          /* matte sigma (float) */
    PBR_TEX_ROUGHNESS = 5,      /* plastic roughness (float) */
    PBR_TEX_SLOTS = 6
};

typedef struct pbr_material_desc {
    int type;                   /* pbr_material_type */
    float Kd[3];                /* matte Kd, plastic Kd */
    float sigma;                /* matte sigma (degrees) */
    float Kr[3];                /* mirror Kr, glass Kr */
    float Kt[3];                /* glass Kt */
    float Ks[3];                /* plastic Ks */
    float eta;                  /* glass index */
    float metal_eta[3];         /* metal eta */
    float metal_k[3];           /* metal k */
    float roughness;            /* metal roughness / plastic roughness */
    float uroughness;           /* glass/metal u roughness (metal: used when has_uv_roughness) */
    float vroughness;
    int has_uv_roughness;       /* metal: uRoughness/vRoughness textures present */
    int remap_roughness;
    int tex[PBR_TEX_SLOTS];     /* pbr_texture_slot → texture index + 1, or 0 (triangle meshes only) */
} pbr_material_desc;

typedef struct pbr_light_desc {
    int type;                   /* pbr_light_type */
    pbr_transform light_to_world;
    float I[3];                 /* point intensity */
    float Le[3];                /* area emission */
    int shape;                  /* area light: index of the mesh shape ... */
    int triangle;               /* ... and the triangle in it */
    int two_sided;
    int n_samples;
    int medium_inside, medium_outside;
    /* SkyBoxLight (Light/SkyBoxLight.h): env data as stbi_loadf returns it with vertical flip */
    float world_center[3];
    float world_radius;
    int env_width, env_height, env_components;
    const float* env_data;      /* env_width*env_height*env_components, or NULL → black */
} pbr_light_desc;

typedef struct pbr_medium_desc {   /* Media/HomogeneousMedium.h */
    float sigma_a[3];
    float sigma_s[3];
    float g;
} pbr_medium_desc;

typedef struct pbr_scene_desc {
    int abi_version;            /* PBR_HIP_ABI_VERSION */
    int n_shapes;
    const pbr_shape_desc* shapes;
    int n_materials;
    const pbr_material_desc* materials;
    int n_lights;
    const pbr_light_desc* lights;
    int n_media;
    const pbr_medium_desc* media;
    int max_prims_in_node;      /* BVHAccel maxPrimsInNode (main.cpp:385 uses 1) */
    int n_textures;
    const pbr_texture_desc* textures;
    int split_method;           /* pbr_split_method (BVHAccel.h:18); Middle / EqualCounts build on the host */
    /* A BVHAccel already built over the primitives IN THE ORDER GIVEN HERE — the reference's own
     * flattened node array (LinearBVHNode, BVHAccel.cpp:46-55, 32 B each), as a Scene's aggregate
     * holds it after its constructor reordered `primitives` into leaf order.  The upload then uses
     * that tree as is instead of building one: the traversal tests the reference's boxes in the
     * reference's order.  It is checked to be a preorder tree whose leaves hold primitives 0..n-1
     * in order, each leaf box the union of its primitives' bounds (PBR_E_INVALID otherwise).
     * NULL = build one (split_method, max_prims_in_node). */
    const void* bvh_nodes;
    int n_bvh_nodes;
} pbr_scene_desc;

/* CreatePerspectiveCamera (Camera/Perspective.cpp:84-104) inputs. */
typedef struct pbr_camera_desc {
    int width, height;          /* raster resolution */
    pbr_transform camera_to_world;
    int use_look_at;            /* if set, camera_to_world = Inverse(LookAt(eye, look, up)) */
    float eye[3], look[3], up[3];
    float fov;                  /* degrees; the reference fixes 90 */
    float lens_radius;          /* the reference fixes 0 */
    float focal_distance;
    int medium;                 /* camera medium (dropped by CameraToWorld, F12) */
    /* 1: raster_to_camera is the camera's own ProjectiveCamera::RasterToCamera (Camera.h:36-53:
     * Inverse(CameraToScreen) · RasterToScreen of its screen window and fov), used instead of
     * CreatePerspectiveCamera's (fov above, the raster's aspect-ratio screen window): a reference
     * PerspectiveCamera built with any fov or screen window (Perspective.cpp:6-9) hands over exactly */
    int use_raster_to_camera;
    pbr_transform raster_to_camera;
} pbr_camera_desc;

typedef struct pbr_tile {
    int x0, y0, x1, y1;         /* half-open pixel rectangle */
} pbr_tile;

typedef struct pbr_render_desc {
    int integrator;             /* pbr_integrator_type */
    int max_depth;
    float rr_threshold;
    int light_strategy;         /* pbr_light_strategy ("spatial" falls back to uniform, LightDistrib.cpp:10-21) */
    int sampler;                /* pbr_sampler_type */
    int spp;
    pbr_camera_desc camera;
    /* pixels to render; n_tiles == 0 → whole frame. Output is packed tile after tile, each tile
     * row-major, 3 floats (linear RGB = colObj/spp) and 4 bytes (RGBA8) per pixel. */
    int n_tiles;
    const pbr_tile* tiles;
    int outputs_on_device;      /* 1: rgb_out/rgba_out are device pointers (e.g. torch tensors) */
    void* stream;               /* hipStream_t to launch on (NULL = context stream).  With
                                 * outputs_on_device, collect_stats == 0 and stats == NULL the call
                                 * is asynchronous: it returns once the frame is enqueued on `stream`
                                 * and the caller synchronises (frames queue back to back). */
    int collect_stats;          /* 1: also count BVH node visits / triangle tests (slower) */
    /* PBR_SAMPLER_SOBOL (pbrt-v3 SobolSampler; the reference ships only its tables, F3):
     * generator matrices in the layout of the reference's SobolMatrices32 (Sampler/SobolMatrices.h:
     * 42-47: [dims][52] uint32 columns).  NULL → the built-in matrices, which are the
     * reference's SobolMatrices32 (all 1024 dimensions, regenerated from the Joe-Kuo direction
     * numbers the table was built from; hash-checked against it).  spp is rounded up to a power of
     * two (GlobalSampler(RoundUpPow2(spp))).  Sample indices are 64-bit as pbrt-v3's: up to 2^52
     * (2·log2(resolution) + log2(spp) <= 52). */
    const uint32_t* sobol_matrices;
    int sobol_dims;
    /* PBR_SAMPLER_TABLE: every sample's dimensions as the caller's sampler gives them —
     * sample_table[((y * camera.width + x) * spp + s) * table_dims + d] = SampleDimension(
     * GetIndexForSample(s), d) at pixel (x, y), host memory, rows of pixels outside the tiles unused.
     * GlobalSampler's bookkeeping (a Get2D at dimension 4 moves to 5, Sampler.cpp:131-143) applies as
     * for the device samplers.  A path that asks for a dimension >= table_dims fails the frame
     * (PBR_E_UNSUPPORTED).  Frames with a table are synchronous; camera.width·height·spp < 2^32. */
    const float* sample_table;
    int table_dims;
} pbr_render_desc;

typedef struct pbr_render_stats {
    double seconds;             /* wall time of the render call (incl. launch + sync) */
    double kernel_ms;           /* device time of the integrator kernel(s), HIP events */
    double film_ms;             /* device time of the film/output kernel */
    uint64_t samples;           /* pixels * spp rendered */
    uint64_t rays;              /* rays traced (closest + any hit), if collect_stats */
    uint64_t node_visits;       /* LinearBVHNode visits, if collect_stats */
    uint64_t prim_tests;        /* primitive intersection tests, if collect_stats */
    uint64_t shading_events;    /* surface/medium interactions shaded, if collect_stats */
    int n_launches;
} pbr_render_stats;

typedef struct pbr_hip_ctx pbr_hip_ctx;

int pbr_hip_create(int device, pbr_hip_ctx** out);
int pbr_hip_upload_scene(pbr_hip_ctx* ctx, const pbr_scene_desc* scene);
int pbr_hip_render(pbr_hip_ctx* ctx, const pbr_render_desc* desc,
                   float* rgb_out, uint8_t* rgba_out, pbr_render_stats* stats);
int pbr_hip_destroy(pbr_hip_ctx* ctx);
const char* pbr_hip_last_error(const pbr_hip_ctx* ctx);
/* Waits for the context's asynchronous frames; returns PBR_E_UNSUPPORTED if one of them stopped at
 * a safety bound (see above). */
int pbr_hip_sync(pbr_hip_ctx* ctx);
/* n frames of one descriptor in one call — SamplerIntegrator::Render (Integrator.cpp:280-356) n
 * times, e.g. the frames of an animation or the timed frames of a benchmark.  The frames' chunks
 * continue one rotation over the chunk lanes with no join between frames, so the launches that end
 * one frame overlap the ones that start the next (a frame of few chunks — a multi-GPU rank's shard —
 * otherwise leaves the GPU part idle at its end).  Every frame is the same bits as pbr_hip_render's.
 * Frame f goes to rgb_outs[f] / rgba_outs[f] (device pointers; either array may be NULL).  Requires
 * desc->outputs_on_device = 1, collect_stats = 0, no sample table.  Asynchronous: returns once the
 * frames are enqueued; desc->stream (NULL: the context stream) reaches its tail when all are done;
 * pbr_hip_wait_frame orders another stream after one frame. */
int pbr_hip_render_frames(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int n, float* const* rgb_outs,
                          uint8_t* const* rgba_outs);
/* Makes `stream` (hipStream_t; NULL = the context stream) wait until frame f of the last
 * pbr_hip_render_frames call is complete (e.g. before gathering it to another GPU). */
int pbr_hip_wait_frame(pbr_hip_ctx* ctx, void* stream, int f);
/* Progressive rendering: a frame's samples in resumable passes over a carried accumulator — what
 * SamplerIntegrator::Render's sample loop (Integrator.cpp:300-312: colObj += Li) holds after some of
 * its iterations.  n_passes passes of samples_per_pass samples per pixel, the first pass starting at
 * sample number first_sample; accum = 6 floats per pixel in the descriptor's packed tile order:
 * Σ Li.rgb and Σ (Li.rgb)² over samples [0, first_sample) on entry (not read when first_sample == 0),
 * over [0, first_sample + n_passes·samples_per_pass) on return.  desc->spp stays the sampler's
 * samplesPerPixel — the whole budget (Sobol: rounded up to a power of two) — and the passes must end
 * at or below it.  The carried sums continue a whole frame's in-order float additions (acc = acc + L,
 * acc2 = acc2 + L·L), so after pass p, with k = first_sample + (p+1)·samples_per_pass samples done,
 * rgb_outs[p] = Σ Li / k is the frame pbr_hip_render gives for a sampler whose samples 0..k-1 are these
 * (Halton: spp = k; Sobol: power-of-two k), and with k = the budget it is pbr_hip_render's bits.
 * rgba_outs[p] is its film transform.  Either array, or any entry, may be NULL to skip that image.
 * The squares serve a per-pixel variance estimate: (Σ L² − (Σ L)²/k) / (k − 1).
 * Conditions as pbr_hip_render_frames: outputs_on_device = 1, collect_stats = 0, accum a device
 * pointer; a sample table returns PBR_E_UNSUPPORTED.  Asynchronous in the same way: passes of one
 * call continue one rotation over the chunk lanes, a pass's write of a pixel's sums ordered after the
 * previous pass's by events; calls on one stream follow each other, and pbr_hip_wait_frame(ctx, stream,
 * p) orders another stream after pass p of the last call. */
int pbr_hip_render_passes(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int first_sample, int samples_per_pass,
                          int n_passes, float* accum, float* const* rgb_outs, uint8_t* const* rgba_outs);

/* ---- adaptive sampling (no reference counterpart) ----
 * Per-pixel stopping over the accumulator of pbr_hip_render_passes.  The rule, for a pixel with k >= 2
 * samples done and sums S_c = Σ L_c, Q_c = Σ L_c² (c = r, g, b), every operation in float32, in this
 * order, nothing fused:
 *     n = (float)k;   m_c = S_c / n;   d_c = Q_c - S_c * m_c;   v_c = d_c > 0 ? d_c : 0   (NaN: 0)
 *     E = ((v_r + v_g) + v_b) / (n * (n - 1))        variance of the pixel mean, summed over channels
 *     M = (m_r + m_g) + m_b;   B = M > floor ? M : floor;   T = tolerance * B
 *     active = E > T * T                              (any NaN: not active)
 * There is no square root and no transcendental in it, so a float32 restatement on the host decides
 * exactly as the device does.  A pixel that is not active has stopped for good.
 *
 * pbr_hip_adaptive_select evaluates the rule over the n_in pixels of list_in (device; ascending packed
 * pixel indices; NULL: all n_pixels, n_in ignored) from accum (device, 6 floats per frame pixel) and
 * writes the active ones, in the same ascending order, to list_out (device, room for as many entries as
 * were considered; not list_in itself) and their number to *n_out (host).  err_out (device, one float per
 * frame pixel, or NULL) receives E of every pixel considered; other entries are not written.  Waits for
 * renders in flight on the context, and is synchronous: it returns *n_out.  PBR_E_INVALID:
 * samples_done < 2, n_pixels outside [1, 2^31), a negative or NaN tolerance or floor, NULL accum, list_out
 * or n_out. */
int pbr_hip_adaptive_select(pbr_hip_ctx* ctx, int64_t n_pixels, int samples_done, float tolerance, float floor, const float* accum,
                            const int32_t* list_in, int n_in, int32_t* list_out, int* n_out, float* err_out);
/* One pass of `samples` samples, numbered from first_sample, for the n_list listed pixels only: list =
 * device, strictly ascending indices into the descriptor's packed tile order (checked on the device:
 * PBR_E_INVALID).  accum, rgb_out and rgba_out are whole-frame buffers in that order (either image may
 * be NULL); a listed pixel ends with exactly what pbr_hip_render_passes would have left there, entries
 * of unlisted pixels are not written.  The list is cut into runs — listed pixels consecutive in one row
 * of one tile — which the pass renders as tiles over a dense copy of the listed sums; the call waits
 * for the run count (one 8-byte copy; this also waits for work queued before it on the stream), then
 * queues the pass as pbr_hip_render_passes does.  Conditions as there: outputs_on_device = 1, no stats,
 * a sample table returns PBR_E_UNSUPPORTED, first_sample + samples within the budget.  n_list == 0 is
 * PBR_OK and launches nothing.  pbr_hip_last_chunks reports the plan for n_list pixels;
 * pbr_hip_wait_frame(ctx, stream, 0) orders another stream after the pass. */
int pbr_hip_render_passes_list(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int first_sample, int samples, const int32_t* list,
                               int n_list, float* accum, float* rgb_out, uint8_t* rgba_out);
typedef struct pbr_adaptive {
    int min_samples;        /* every pixel takes these first: 2 <= min_samples <= budget */
    int samples_per_round;  /* what the pixels still active take per round, >= 1 */
    float tolerance;        /* relative error of the pixel mean at which a pixel stops, >= 0 */
    float floor;            /* lower bound of the mean the tolerance is relative to, >= 0 */
} pbr_adaptive;
typedef struct pbr_adaptive_result {
    int rounds;             /* passes rendered, the full-frame first one included */
    int max_samples_done;   /* the largest count any pixel reached */
    int64_t samples;        /* Σ counts */
    int64_t active_at_end;  /* pixels the last select still found active (they stopped at the budget) */
} pbr_adaptive_result;
/* A whole adaptive render; desc->spp is the budget (Sobol: rounded up to a power of two, as for passes).
 * Every pixel takes min_samples samples (a plain full-frame pass); then, with k samples done by the
 * pixels still listed: select over the list at k; stop if nothing is active or k is the budget; else the
 * active pixels take min(samples_per_round, budget - k) more.  On return counts[p] (device, int32 per
 * pixel) is the number of samples pixel p took, accum[p] its sums over exactly those samples, rgb_out[p]
 * and rgba_out[p] (either may be NULL) its image at that count: the bits pbr_hip_render_passes leaves
 * at that count.  A Sobol image at a count that is not a power of two has no reference counterpart; the
 * call is allowed all the same.  Synchronous: each round waits for one 8-byte copy (active pixels, runs)
 * before it queues the round's pass, and the call returns when the last round is done.  The library
 * keeps no state between calls: a checkpoint is accum plus counts.  `result` may be NULL. */
int pbr_hip_render_adaptive(pbr_hip_ctx* ctx, const pbr_render_desc* desc, const pbr_adaptive* params, float* accum, int32_t* counts,
                            float* rgb_out, uint8_t* rgba_out, pbr_adaptive_result* result);

/* ---- feature buffers (no reference counterpart) ----
 * The side inputs a denoiser asks for beside a low-sample image: per pixel the albedo, normal and depth
 * of the first surface each camera sample sees, summed over the same camera samples as the beauty image
 * of pbr_hip_render_passes.  For pixel p and sample number s the sampler is positioned exactly as a
 * render positions it (the sample index of (x, y, s), dimensions 0-4 through GetCameraSample, thin lens
 * included; the render's own camera function).  The camera ray is traced to its closest hit.  A hit on a
 * surface without a material is a medium boundary (the !isect.bsdf case of the three Li's) and is passed
 * through as Li passes it — SpawnRay(ray.d), trace again — up to 1024 crossings; beyond that the frame
 * fails through the device guard (PBR_E_UNSUPPORTED from this call or the next pbr_hip_sync), as a
 * render does.  The sample's eight values (all 0 on a miss):
 *     0-2  albedo, float32, nothing fused, from the material's parameters after their textures are
 *          evaluated at the hit's (u, v) and after the material's own clamp to [0, inf): Matte Kd,
 *          Plastic Kd, Mirror Kr, Glass Kt; Metal the conductor's reflectance at normal incidence per
 *          channel, in this order: a = eta - 1; b = eta + 1; k2 = k * k; r = (a * a + k2) / (b * b + k2).
 *          A sphere uses its material's constants.
 *     3    hit: 1.0f
 *     4-6  the shading normal ns of pbr_surface_hit: world space, as the intersection leaves it, not
 *          flipped towards the camera
 *     7    t: the ray parameter of the recorded hit; with crossings, the sum of the segments' t in order
 *          (camera directions are unit length, so a distance)
 * accum = PBR_AOV_CHANNELS floats per pixel in the descriptor's packed tile order.  A pass over samples
 * [first_sample, first_sample + samples) continues each channel's sum in sample order with acc = acc + v
 * (the rule of pbr_hip_render_passes), so any cut of the samples into passes leaves the bits of one
 * pass; with first_sample == 0 accum is not read.  aov_out (or NULL) receives the image, 8 floats per
 * pixel, with k = first_sample + samples samples done: channels 0-2 Σalbedo / k; 3 Σhit / k, the
 * coverage; 4-6 Σns / k — an average, NOT renormalised to unit length; 7 Σt / Σhit where Σhit > 0, else 0.
 * Conditions as pbr_hip_render_passes: outputs_on_device = 1, collect_stats = 0, accum a device pointer,
 * aov_out a device pointer or NULL; a sample table returns PBR_E_UNSUPPORTED; desc->spp is the sampler's
 * budget (Sobol: rounded up to a power of two) and first_sample + samples must not exceed it.  The
 * descriptor's integrator, depth, roulette and light strategy are ignored; its camera, sampler, spp and
 * tiles are used.  Asynchronous on desc->stream with the ordering of a pass: calls on one stream follow
 * each other, a call on another stream drains the context first, and pbr_hip_wait_frame(ctx, stream, 0)
 * orders another stream after the call.  PBR_E_INVALID: NULL ctx, desc or accum, samples < 1,
 * first_sample < 0, a range above the budget.  A scene whose tree is too deep for the quad walk runs the
 * per-lane binary walk. */
#define PBR_AOV_CHANNELS 8
int pbr_hip_render_aov(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int first_sample, int samples, float* accum, float* aov_out);
/* How such a pass over n_pixels pixels is cut into kernel launches (a pure function: no context, no GPU
 * call): consecutive ranges of the packed pixel order, each launch below 2^31 samples (C4's 8,294,400
 * pixels at 1024 samples take four).  Up to max_launches ranges go to first_pixel[] / n_launch_pixels[]
 * (either may be NULL when max_launches == 0); *n_launches is their total number. */
int pbr_hip_plan_aov(int64_t n_pixels, int samples, int max_launches, int64_t* first_pixel, int64_t* n_launch_pixels,
                     int* n_launches);
/* The feature pass with mirror bounces followed, so that a mirror reports what it reflects.
 * max_bounces == 0 is pbr_hip_render_aov in every respect (that call is this one with 0); outside 0..16:
 * PBR_E_INVALID.  Buffers, passes, tiles, streams, ordering, the crossing guard and the other refusals are
 * those of pbr_hip_render_aov.  Per sample, with max_bounces = B > 0:
 *   The chain.  The camera ray is traced as above, through material-less surfaces, to a hit with a BSDF:
 *   surface 1.  At surface j a mirror step is taken when j <= B, the material is PBR_MAT_MIRROR, and
 *   Whitted's SpecularReflect would continue there: Sample_f of the specular reflection lobe on the hit's
 *   frame (ss = normalize(dpdu), ts = cross(ns, ss)) gives a non-black f (Kr after its texture and clamp is
 *   not all zero), pdf > 0 (wo is not in the shading tangent plane) and absdot(wi, ns) != 0.  The lobe is
 *   deterministic, wi = (-wo.x, -wo.y, wo.z) in that frame, and no sampler dimension is read, so the chain
 *   is that of Whitted, Path and VolPath alike.  Glass and glossy lobes are not followed.
 *   The continuation is SpawnRay(isect, wi) (pbr_hip_mirror_step_host gives its bits; pbr_hip_bsdf with
 *   PBR_BSDF_MIRROR reports the direction as s_wi), traced again through material-less surfaces; the
 *   1024-crossing bound counts over the whole chain.
 *   The recorded surface is the last surface with a BSDF the chain reached: the first one where no step is
 *   taken (not a mirror, the step refused, or B steps taken), or, when a continuation misses the scene, the
 *   mirror it left (crossings made after that mirror do not count towards its distance).
 *   The eight values (all 0 when the camera ray itself misses):
 *     0-2  a = alb_1; a = a * alb_2; ... per channel, float32, in chain order up to and including the
 *          recorded surface; each alb is the albedo defined above at that hit (a mirror's: Kr)
 *     3    1.0f
 *     4-6  ns of the recorded surface, world space, as the intersection leaves it.  It is NOT reflected
 *          back through the mirrors: in a planar mirror it is the normal of the real surface, not of its
 *          mirror image
 *     7    T at the recorded surface, T = T + t over every segment up to it, in order, float32
 * For a planar mirror eye + d * T is the mirror image of the recorded point, which is the point whose
 * reprojection pbr_hip_temporal needs; for a curved mirror the chain is followed all the same, but that
 * identity does not hold.  Sums, passes, the image formula and the launch plan are unchanged. */
int pbr_hip_render_aov_mirrors(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int max_bounces, int first_sample, int samples,
                               float* accum, float* aov_out);

/* ---- denoise (no reference counterpart) ----
 * An edge-avoiding à-trous filter (Dammertz et al. 2010; the spatial part of SVGF, Schied et al. 2017)
 * over what the passes leave on the device: the six sums per pixel of pbr_hip_render_passes (accum), the
 * 8-float image pbr_hip_render_aov writes to aov_out (aov), and optionally the per-pixel sample counts
 * of pbr_hip_render_adaptive (counts; NULL: every pixel took `samples`).  A 5x5 B3-spline wavelet,
 * `iterations` levels, level i stepping 2^i pixels, with edge stopping on the luminance scaled by the
 * locally blurred variance of the pixel mean, on the mean shading normal and on the distance scaled by its
 * screen-space slope; the variance is carried from level to level.  With demodulate the colour is divided
 * by the first-hit albedo (1 where the samples missed) before the filter and multiplied back after it.
 * Every operation is float32 in the order DESIGN §4.5 states, nothing fused, no transcendental: the
 * result is pinned bit for bit by a float32 restatement (tests/denoise_expected.py).
 * Buffers are device pointers over a frame in raster order, row 0 first (what a descriptor with
 * n_tiles == 0 renders).  Outputs, each may be NULL but not all three: rgb_out 3 floats per pixel;
 * rgba_out the film transform of rgb_out (the 8-bit pixels of a render); var_out 1 float per pixel, the
 * filtered variance in the filter's domain (after demodulation, summed over the channels).
 * Asynchronous on `stream` (NULL: the context's) with the ordering of pbr_hip_render_aov: calls on one
 * stream follow each other, a call on another stream drains the context first, and
 * pbr_hip_wait_frame(ctx, stream, 0) orders another stream after the call.  The working planes (64 bytes
 * per pixel) live in the context: allocated on first use, grown when the frame grows, freed by
 * pbr_hip_destroy.  No scene is needed.
 * PBR_E_INVALID: NULL ctx, p, accum or aov; all outputs NULL; width or height < 1; width * height >= 2^31;
 * iterations outside 1..8; a sigma that is <= 0 or NaN; counts == NULL with samples < 2. */
typedef struct pbr_denoise {
    int width, height;     /* the frame: buffers are row-major, row 0 first */
    int iterations;        /* 1..8 levels; level i steps 2^i pixels */
    int demodulate;        /* 1: filter colour / albedo and multiply back */
    float sigma_l, sigma_n, sigma_z;   /* > 0, +inf switches a term off; suggested defaults 4, 0.4, 1 */
} pbr_denoise;
int pbr_hip_denoise(pbr_hip_ctx* ctx, const pbr_denoise* p, int samples, const int32_t* counts, const float* accum,
                    const float* aov, float* rgb_out, uint8_t* rgba_out, float* var_out, void* stream);

/* ---- the denoiser's spatial variance estimate (no reference counterpart) ----
 * pbr_hip_denoise forms a pixel's variance from its own two sums, so a pixel with one sample has none
 * (V = 0) and the luminance edge-stop drops every neighbour that is not equal: a 1-sample frame comes back
 * as it went in.  The estimate (SVGF, Schied et al. 2017, §4.2) runs between prepare and level 0: a pixel
 * with 1 <= count < min_count takes its variance from the first and second moments of the pixels in a
 * (2·radius+1)² window around it, each weighted by its count times the filter's normal and depth edge-stops
 * at step 1 (no luminance term), as the variance of a mean of its own `count` samples; a pixel whose kept
 * neighbours hold fewer than two samples, and every pixel with count 0 or >= min_count, keeps prepare's
 * variance.  The colour is not changed; the levels and the finish run as in pbr_hip_denoise.  Float32 in the
 * order DESIGN §4.9 states, pinned bit for bit by tests/spatial_variance_expected.py.
 *
 * pbr_hip_denoise_sv: sv == NULL is pbr_hip_denoise in every respect (which is a call of it).  With sv,
 * counts == NULL with samples == 1 is allowed; everything else — buffers, outputs, ordering, streams — is as
 * for pbr_hip_denoise.  The estimate needs a fifth working plane (16 bytes per pixel), allocated by the
 * first call that passes sv.
 * PBR_E_INVALID: as pbr_hip_denoise, but with sv samples < 1 (not < 2) when counts == NULL; min_count outside
 * 2..64; radius outside 1..3.
 *
 * pbr_hip_spatial_variance_host: prepare and the estimate — the device's per-pixel functions compiled for
 * the host — over host pointers; var_out, 1 float per pixel (required), is the variance plane level 0 would
 * read.  sv == NULL gives prepare's variance.  No context, no GPU call; the same refusals. */
typedef struct pbr_spatial_variance {
    int min_count;  /* 2..64: a pixel with 1 <= count < min_count takes the spatial estimate; suggested 4 */
    int radius;     /* 1..3: the window is (2·radius+1)² pixels; suggested 1 */
} pbr_spatial_variance;
int pbr_hip_denoise_sv(pbr_hip_ctx* ctx, const pbr_denoise* p, const pbr_spatial_variance* sv, int samples,
                       const int32_t* counts, const float* accum, const float* aov, float* rgb_out, uint8_t* rgba_out,
                       float* var_out, void* stream);
int pbr_hip_spatial_variance_host(const pbr_denoise* p, const pbr_spatial_variance* sv, int samples, const int32_t* counts,
                                  const float* accum, const float* aov, float* var_out);

/* ---- temporal accumulation (no reference counterpart) ----
 * The temporal part of SVGF (Schied et al. 2017) as a merge of accumulators: the previous frame's sums are
 * carried into this frame's, so that a moving camera at a few samples per frame does not start from nothing.
 * Per pixel that hit something, the point its centre sees (the pinhole ray through the centre at the mean
 * first-hit distance) is projected into the previous frame; the previous frame's per-sample means of L and L²
 * are resampled there over the four surrounding pixels, each tap kept only where the previous frame saw a
 * surface at the expected distance (tol_z, relative) with about the same mean normal (tol_n, squared
 * difference) and holds finite sums; with demodulate the taps are resampled as colour / first-hit albedo and
 * multiplied by this pixel's albedo.  The history enters as min(the taps' smallest count, max_history)
 * samples: accum_out = accum_cur + history mean * that number, counts_out = count + that number, the format
 * of accum and counts, so pbr_hip_denoise(counts = counts_out) and the variance estimate work on it
 * unchanged.  A pixel without a hit, off the previous frame, behind the previous camera or without a valid
 * tap keeps its own sums bit for bit.  Static scenes only: a moving object is not reprojected.  Every
 * operation is float32 in the order DESIGN §4.8 states, nothing fused, no transcendental: the result is
 * pinned bit for bit by a float32 restatement (tests/temporal_expected.py).
 *
 * pbr_hip_camera_matrices: the two matrices and the eye point such a call needs, from build_camera's own
 * transforms of a descriptor (use_look_at and use_raster_to_camera honoured, lens_radius ignored), row
 * major: raster_to_world = CameraToWorld · RasterToCamera, world_to_raster its inverse (the product of the
 * stored inverses, no new inversion), eye = CameraToWorld applied to the origin.  Host only: no context, no
 * GPU call.  PBR_E_INVALID: a NULL argument, width or height < 1.
 *
 * pbr_hip_temporal.  Buffers are device pointers over a width x height frame in raster order, row 0 first:
 * accum_* 6 floats per pixel (the sums of pbr_hip_render_passes), aov_* the 8-float image of
 * pbr_hip_render_aov, counts_prev (required) the samples behind each previous pixel, counts_cur the samples
 * behind each current pixel (NULL: every pixel took `samples`; entries below 2^30 — the caller's contract).
 * accum_out and counts_out are required; motion_out (2 floats per pixel: the pixel's raster position in the
 * previous frame minus its position in this one, (0, 0) without a projection), rgb_out (accum_out's colour
 * sum / counts_out, 0 where the count is 0) and rgba_out (its film transform) may each be NULL.  accum_out
 * may be accum_cur and counts_out may be counts_cur (a pixel reads only its own current entry); an output
 * pointer equal to counts_prev, accum_prev or aov_prev returns PBR_E_INVALID.  Asynchronous on `stream`
 * (NULL: the context's) with the ordering of pbr_hip_denoise: calls on one stream follow each other, a call
 * on another stream drains the context first, and pbr_hip_wait_frame(ctx, stream, 0) orders another stream
 * after the call.  No scene is needed and nothing is allocated.
 * PBR_E_INVALID: NULL ctx, p or a required buffer; width or height < 1; width * height >= 2^31; max_history
 * outside 1..2^20; tol_z or tol_n negative or NaN; counts_cur == NULL with samples < 1; a NaN in either
 * matrix or eye; the aliasing above.
 *
 * pbr_hip_temporal_host: the same per-pixel function compiled for the host, over host pointers, without the
 * images; no context, no GPU call; the same refusals. */
int pbr_hip_camera_matrices(const pbr_camera_desc* cam, float raster_to_world[16], float world_to_raster[16], float eye[3]);
typedef struct pbr_temporal {
    int width, height;          /* whole frame, raster order, row 0 first (as pbr_denoise) */
    int max_history;            /* 1 .. 2^20: cap, in samples, of the history a pixel takes over */
    int demodulate;             /* 1: history is resampled as colour / first-hit albedo */
    float tol_z;                /* >= 0: relative distance tolerance of a tap; suggested 0.05 */
    float tol_n;                /* >= 0: squared difference of the mean normals; suggested 0.1 */
    float cur_raster_to_world[16];
    float cur_eye[3];
    float prev_world_to_raster[16];
    float prev_eye[3];
} pbr_temporal;
int pbr_hip_temporal(pbr_hip_ctx* ctx, const pbr_temporal* p, int samples, const int32_t* counts_cur, const float* accum_cur,
                     const float* aov_cur, const int32_t* counts_prev, const float* accum_prev, const float* aov_prev,
                     float* accum_out, int32_t* counts_out, float* motion_out, float* rgb_out, uint8_t* rgba_out, void* stream);
int pbr_hip_temporal_host(const pbr_temporal* p, int samples, const int32_t* counts_cur, const float* accum_cur,
                          const float* aov_cur, const int32_t* counts_prev, const float* accum_prev, const float* aov_prev,
                          float* accum_out, int32_t* counts_out, float* motion_out);

/* ---- schedule (no reference counterpart) ----
 * How a frame is cut into launches on the device.  Every setting renders the same bits (the GPU
 * tests compare them with each other and with the reference); the defaults — a zeroed struct or
 * NULL — are the measured schedule of DESIGN.md §4.  The library reads no environment variables:
 * this call is the only run-time switch.  The setting holds for the context's later renders. */
enum pbr_kernels_mode {
    PBR_KERNELS_AUTO = 0,       /* the wavefront schedule wherever the integrator and scene allow it */
    PBR_KERNELS_MEGAKERNEL = 1  /* one kernel per frame, whole Li per lane */
};
enum pbr_fuse_mode {
    PBR_FUSE_AUTO = 0,          /* Whitted's level-0 shade traces its own camera rays in frames of at
                                 * least max(2, lanes) chunks (a separate camera kernel otherwise) */
    PBR_FUSE_OFF = 1,
    PBR_FUSE_ON = 2
};
typedef struct pbr_schedule {
    int kernels;                /* pbr_kernels_mode */
    int chunk_log2;             /* at most 2^chunk_log2 samples per chunk (10..28; 0 = the default: 25 for
                                 * Whitted, less with several lights; for Path / VolPath the largest of
                                 * 2^20..2^27 whose lanes' queues fit 3/4 of the device memory free or held
                                 * by the context — 2^26 on 3 lanes when that memory cannot be queried; Whitted's
                                 * default shrinks in the same way on a device with less room than its lanes
                                 * need); capped at 25 (Whitted) and 27 (Path / VolPath).  24 or more chunks are
                                 * made equal, a whole number per lane: see pbr_hip_plan_chunks */
    int lanes;                  /* chunk lanes, each its own stream and queues (1..4); 0 = 3 (Path: 4 where
                                 * four lanes of 2^27-sample chunks fit the memory share above) */
    int fuse_camera;            /* pbr_fuse_mode */
    int serial;                 /* 1: every launch of a frame on the caller's stream, one after another
                                 * (one lane, no shadow stream) — measures each kernel on its own */
} pbr_schedule;
int pbr_hip_set_schedule(pbr_hip_ctx* ctx, const pbr_schedule* sched);

/* ---- the chunk plan (no reference counterpart) ----
 * How the wavefront schedules cut a frame into chunks over lanes: a pure function of the schedule
 * request, the frame and the memory the lanes may take.  The renders take every chunking decision
 * from it, so a test (or a caller sizing its own buffers) can ask for the plan instead of restating
 * the rule. */
typedef struct pbr_chunk_query {
    int integrator;             /* pbr_integrator_type */
    int64_t n_pixels;           /* pixels of the frame (the sum of its tiles) */
    int spp;                    /* samples per pixel of one frame (render_passes: of one pass) */
    int max_depth;
    int n_lights;               /* lights of the scene */
    int sky_light;              /* 1: the scene's single light is a SkyBox */
    int batch;                  /* 1: pbr_hip_render_frames / pbr_hip_render_passes, 0: pbr_hip_render */
    int scene_fusable;          /* 1: the scene's materials allow Whitted's fused level-0 shade (untextured
                                 * matte / mirror / simple lobes, few enough to stage in LDS) */
    double lane_budget;         /* bytes the lanes' buffers may take: 3/4 of the device memory free or held
                                 * by the context's lanes; 0 = unknown (the memory query failed): Whitted
                                 * keeps its default chunk, Path / VolPath plan 2^26-sample chunks on 3 lanes */
} pbr_chunk_query;
typedef struct pbr_chunk_plan {
    int lanes;                  /* 1..4; 0 (with n_chunks 0): the call ran the megakernel, which has no chunks */
    int chunk_log2;             /* the chosen bound: at most 2^chunk_log2 samples per chunk */
    int64_t chunk_pixels;       /* chunk c covers packed pixels [c·chunk_pixels, min((c+1)·chunk_pixels, n_pixels)) */
    int64_t n_chunks;
    uint64_t cap;               /* samples of a whole chunk: chunk_pixels · spp */
    uint64_t qcap;              /* entries of a lane's queues: >= cap and >= seg_cap · PBR_WALK_SEGMENTS */
    int seg_cap;                /* entries of one queue segment (a multiple of 256) */
    int lane0_on_ctx_stream;    /* pbr_hip_last_chunks: 1 when lane 0 ran on the context's stream and not on the
                                 * caller's (four lanes and a caller's stream) */
    int fused_camera;           /* Whitted: the level-0 shade traced its own camera rays */
    int reserved;
    double bytes_per_sample;    /* estimate of one lane's buffers per queue entry; an upper bound:
                                 * lanes · bytes_per_sample · qcap >= what the lanes allocate */
    double lane_budget;         /* the budget the plan was made for */
    uint64_t held_lane_bytes;   /* pbr_hip_last_chunks: bytes the context's lane buffers hold (they grow to the
                                 * largest plan rendered and are never shrunk) */
} pbr_chunk_plan;
/* The plan for `query` under `sched` (NULL = the defaults).  No context, no GPU call.  PBR_E_INVALID:
 * a NULL query or out, an unknown integrator, n_pixels or spp < 1, a schedule pbr_hip_set_schedule
 * would reject. */
int pbr_hip_plan_chunks(const pbr_schedule* sched, const pbr_chunk_query* query, pbr_chunk_plan* out);
/* The plan the context's last pbr_hip_render, pbr_hip_render_frames or pbr_hip_render_passes call ran,
 * with the budget computed for that call and the bytes the lane buffers hold after it. */
int pbr_hip_last_chunks(pbr_hip_ctx* ctx, pbr_chunk_plan* out);

/* ---- per-kernel profile (measurement; no reference counterpart) ----
 * While profiling is on, every kernel launch of a render is bracketed by a HIP event pair on the
 * stream it runs on, and each kernel family counts the work units it processed.  `bytes` is the
 * family's ALGORITHMIC HBM traffic: the compulsory queue / per-sample record / output bytes of the
 * wavefront design per counted unit — BVH, mesh and texture fetches, which the
 * caches serve, are not counted. */
typedef struct pbr_kernel_profile {
    char name[40];              /* kernel family, e.g. "k_wf_shade" (rocprof adds template args) */
    int launches;
    double ms;                  /* summed HIP-event durations of the family's launches */
    uint64_t units;             /* work units: samples (camera), queued rays, pixels (finish) */
    uint64_t bytes;             /* algorithmic HBM bytes */
    uint64_t counts[8];         /* raw counters: [0] units, [1..4] pushes / rays that got through */
} pbr_kernel_profile;
/* on = 1: start a measurement window of event timings; on = 2: timings and work counters (the
 * counters add one small counting launch after each queue kernel); 0: stop.  Either resets. */
int pbr_hip_set_profiling(pbr_hip_ctx* ctx, int on);
/* Waits for the context's work, returns the window's per-family profile (n = families seen; at most
 * `max` written) and starts a new window. */
int pbr_hip_get_profile(pbr_hip_ctx* ctx, pbr_kernel_profile* out, int max, int* n);

/* ---- introspection used by the parity tests (no reference counterpart) ---- */
/* Flattened BVH after upload: 32-B LinearBVHNode records (BVHAccel.cpp:46-55) and the ordered
 * primitive ids (position in the `prims` vector).  Pass NULL buffers to query counts. */
int pbr_hip_get_bvh(pbr_hip_ctx* ctx, void* nodes_out, int* n_nodes, int32_t* prim_ids_out, int* n_prims);
/* Halton/Sobol samples computed ON THE DEVICE for (pixel, sample, dim) triples. */
int pbr_hip_sampler_values(pbr_hip_ctx* ctx, int sampler, int width, int height, int spp,
                           int n, const int32_t* px_py_sample_dim, float* out);
/* GlobalSampler::GetIndexForSample (Sampler.h:69; Halton.cpp:61-81, pbrt-v3 SobolSampler) on the
 * device: px_py_sample = 3 ints per query, out = the 64-bit interval sample index. */
int pbr_hip_sample_index(pbr_hip_ctx* ctx, int sampler, int width, int height, int spp, int n,
                         const int32_t* px_py_sample, int64_t* out);
/* GlobalSampler::SampleDimension(index, dimension) (Sampler.h:70; Halton.cpp:83-92, pbrt-v3
 * SobolSampler, whose dimensions 0 and 1 are taken relative to the current pixel: px_py_dim = 3 ints
 * per query, pixel then dimension). */
int pbr_hip_sample_dimensions(pbr_hip_ctx* ctx, int sampler, int width, int height, int n, const int64_t* index,
                              const int32_t* px_py_dim, float* out);
/* Camera rays computed on the device for raster samples (pFilm.x, pFilm.y): out = o.xyz, d.xyz */
int pbr_hip_camera_rays(pbr_hip_ctx* ctx, const pbr_camera_desc* cam, int n, const float* pfilm, float* out);
/* Closest-hit queries on the device: rays = o.xyz d.xyz tmax; out = {hit, t, prim_id, b1, b2} as floats */
int pbr_hip_intersect(pbr_hip_ctx* ctx, int n, const float* rays, float* out, int any_hit);
/* The same queries through one of the BVH walks the render schedules run (rays and out as above;
 * every walk returns the records pbr_hip_intersect returns).  Each value runs the walk with the
 * template arguments and launch bounds of its production users. */
enum pbr_walk {
    PBR_WALK_LANE = 0,       /* what pbr_hip_intersect runs: the per-lane quad walk, private stack */
    PBR_WALK_LANE_LDS = 1,   /* the per-lane quad walk with the LDS short stack (Whitted's shadow kernels) */
    PBR_WALK_PACKET = 2,     /* the wave-packet walk (camera kernels; Whitted's extend when a queue is given);
                              * closest hit only: PBR_E_UNSUPPORTED with any_hit */
    PBR_WALK_REFILL = 3,     /* lane refill over a segmented queue: closest hit (Path's extend and probe kernels)
                              * or any hit (Path's shadow kernel) */
    PBR_WALK_BINARY = 4,     /* the binary walk of trees too deep for the quad walk's stack */
    PBR_WALK_REFILL_TR = 5   /* lane refill as VolPath's transmittance kernel instantiates it; any hit only:
                              * PBR_E_UNSUPPORTED without any_hit */
};
/* The queue walks (PBR_WALK_REFILL, PBR_WALK_REFILL_TR, and PBR_WALK_PACKET when seg_cap > 0 or
 * seg_counts is given, which runs Whitted's extend kernel) lay the rays out as a segmented queue of
 * PBR_WALK_SEGMENTS segments of seg_cap entries: seg_counts[s] rays in segment s, ray i at the i-th
 * dense position; seg_counts = NULL fills the segments in order (the densest prefix), seg_cap = 0
 * picks a capacity.  The other walks take seg_cap = 0 and seg_counts = NULL.  PBR_E_INVALID: an
 * unknown walk, counts that do not sum to n or exceed seg_cap, a queue above 256 MB.
 * PBR_E_UNSUPPORTED: a quad, packet or refill walk on a scene whose tree is walked in binary form
 * (the quad walk's stack cannot hold it), or a walk that reached a safety bound. */
#define PBR_WALK_SEGMENTS 2048
int pbr_hip_intersect_walk(pbr_hip_ctx* ctx, int walk, int n, const float* rays, float* out, int any_hit,
                           int seg_cap, const int32_t* seg_counts);
/* ---- the reference's C++ query surface, batched (include/pbr/pbr.h builds on these) ---- */
/* SurfaceInteraction fields of a hit (Core/Interaction.h:56-105), as GeometricPrimitive::Intersect
 * leaves them (Primitive.cpp:22-36): t = the ray's new tMax. */
typedef struct pbr_surface_hit {
    int hit;                    /* 0 / 1 */
    int prim;                   /* index in the prims vector (shape order), -1 on a miss */
    float t;
    float b[3];                 /* barycentrics of the watertight test (triangles; 0 for spheres) */
    float p[3], p_error[3];
    float n[3];                 /* geometric normal (Triangle.cpp:182-184 orientation rules; on a mesh with
                                 * normals turned to ns's side, Interaction.cpp:104-105) */
    float ns[3], dpdu[3];       /* shading frame after the per-vertex normals (Triangle.cpp:186-253) */
    float wo[3];
    float uv[2];                /* surface (u, v) of the hit (Triangle.cpp:160-190; sphere: phi/phiMax, (theta-thetaMin)/range) */
    int medium_inside, medium_outside;   /* the primitive's MediumInterface (indices, -1 = none) */
} pbr_surface_hit;
/* Scene::Intersect (Core/Scene.cpp:20-24) or, with any_hit, IntersectP (:26-28) for n rays
 * (7 floats each: o.xyz, d.xyz, tMax).  prim >= 0 restricts the query to that one primitive
 * (GeometricPrimitive::Intersect / IntersectP, Core/Primitive.cpp:22-44).  Any-hit queries fill
 * only `hit`. */
int pbr_hip_query(pbr_hip_ctx* ctx, int n, const float* rays, int any_hit, int prim, pbr_surface_hit* out);
/* World bounds (lo.xyz, hi.xyz): prim = -1 → Scene::WorldBound (the BVH root, Scene.cpp:7-17);
 * prim >= 0 → GeometricPrimitive::WorldBound of that primitive (Primitive.cpp:18-20). */
int pbr_hip_bounds(pbr_hip_ctx* ctx, int prim, float* out6);
/* SamplerIntegrator::Li (Integrator.h:44) for n rays (7 floats each) on the device, with the
 * integrator / sampler / light strategy of `desc` (its tiles and outputs are ignored): each ray's
 * sampler is GlobalSampler-positioned at (pixel x, y; sample s) with its next dimension `dim`
 * (px_py_sample_dim: 4 ints per ray; dim 5 after GetCameraSample of a pinhole camera).  depth is
 * the recursion depth argument (Whitted).  rgb_out: 3 floats per ray. */
int pbr_hip_li(pbr_hip_ctx* ctx, const pbr_render_desc* desc, int n, const float* rays,
               const int32_t* px_py_sample_dim, int depth, float* rgb_out);

/* ---- the scattering layer on caller-given directions ----
 * BSDF::f, Pdf and Sample_f (Material/Reflection.cpp:56-164) of the uploaded scene's materials, one
 * query per lane, through the functions the shading kernels call (pbr_device.h bsdf_f, bsdf_pdf,
 * bsdf_f_pdf, bsdf_sample, bsdf_sample_dir + bsdf_sample_sum).  The BSDF is built as
 * ComputeScatteringFunctions builds it at a hit: lobe template 2 * material + multi_lobe, frame
 * ss = normalize(dpdu), ts = cross(ns, ss).  All directions are world directions. */
typedef struct pbr_bsdf_query {
    int material;               /* index into the scene's materials; outside it, or PBR_MAT_NONE: no BSDF */
    int multi_lobe;             /* allowMultipleLobes (Whitted 0, Path / VolPath 1) */
    int type;                   /* BxDFType mask (BSDF_REFLECTION 1, TRANSMISSION 2, DIFFUSE 4, GLOSSY 8, SPECULAR 16) */
    int pad0;
    float n[3], ns[3], dpdu[3]; /* geometric normal, shading normal, shading dpdu */
    float uv[2];                /* surface (u, v): read by image-textured materials only */
    float wo[3], wi[3];
    float u0, u1;               /* the sample of Sample_f */
    float pad1;
} pbr_bsdf_query;
/* pdf and sampled type are set to -1 before each sample call, wi to 0: BSDF::Sample_f leaves *pdf
 * (and the type) untouched when wo lies in the shading tangent plane (Reflection.cpp:121), and so
 * does the record.  wi is meaningful only where the sample's pdf is not 0. */
typedef struct pbr_bsdf_record {
    int no_bsdf;                /* 1: material == nullptr or out of range; every other field is 0 */
    float f[3];                 /* bsdf_f */
    float pdf;                  /* bsdf_pdf */
    float f_lam[3], pdf_lam;    /* bsdf_f_pdf given Lambda(wo) (mf_lambda), as Path and VolPath call it */
    float f_nolam[3], pdf_nolam;/* bsdf_f_pdf without it */
    float s_wi[3], s_f[3], s_pdf;   /* bsdf_sample */
    int s_type;
    float d_wi[3], d_f[3], d_pdf;   /* bsdf_sample_dir given Lambda(wo), then bsdf_sample_sum */
    int d_type;
    int d_ok;                   /* what bsdf_sample_dir returned; 0: the sum was not formed (d_f = 0) */
    int pad[2];
} pbr_bsdf_record;
/* The instantiation evaluated: the lobe mask a production shading kernel is compiled under (kinds
 * outside it compile out) and where it reads the lobe templates.  A mask that does not cover the
 * scene's lobe kinds is refused (PBR_E_INVALID): no render launches that, and its result is
 * meaningless.  The probe kernel is compiled apart from the shading kernels; the library is built
 * without contraction or fast-math and with correctly rounded division and square root, so the
 * source and the mask fix every bit, and the probe's bits are the shading kernels'. */
enum pbr_bsdf_variant {
    PBR_BSDF_ALL = 0,           /* every lobe kind; templates from LDS when they fit (32), else global memory */
    PBR_BSDF_SIMPLE = 1,        /* Lambert, Oren-Nayar, specular (Whitted / Path without microfacets) */
    PBR_BSDF_MATTE_MIRROR = 2,  /* Lambert + mirror (C2, C3) */
    PBR_BSDF_MICRO = 3,         /* Lambert + microfacet reflection / transmission (C4, C5) */
    PBR_BSDF_PASS_L = 4,        /* the classed shade's passes: Lambert */
    PBR_BSDF_PASS_R = 5,        /* microfacet reflection */
    PBR_BSDF_PASS_LR = 6,       /* Lambert + microfacet reflection */
    PBR_BSDF_PASS_RT = 7,       /* microfacet reflection + transmission */
    PBR_BSDF_PASS_LRT = 8,      /* = PBR_BSDF_MICRO's mask, as the last pass instantiates it */
    PBR_BSDF_MIRROR = 9,        /* specular reflection alone (Whitted's mirror bounce) */
    PBR_BSDF_TEXTURED = 10,     /* every kind, image-textured materials' lobes built per hit; global memory */
    PBR_BSDF_ALL_LDS = 11,      /* every kind, templates from the LDS copy (PBR_E_INVALID above 32 templates) */
    PBR_BSDF_ALL_GLOBAL = 12    /* every kind, templates from global memory */
};
int pbr_hip_bsdf(pbr_hip_ctx* ctx, int variant, int n, const pbr_bsdf_query* queries, pbr_bsdf_record* out);
/* The same functions compiled for the host, for one material with constant textures (query material
 * 0; any other index: no BSDF), through the conversion pbr_hip_upload_scene applies to it.  No
 * context, no GPU.  PBR_E_INVALID: an image-textured or unknown material, an unknown variant, a
 * mask that does not cover the material's lobes. */
int pbr_hip_bsdf_host(const pbr_material_desc* material, int variant, int n, const pbr_bsdf_query* queries,
                      pbr_bsdf_record* out);
/* One mirror step of pbr_hip_render_aov_mirrors per hit, through the function its kernel calls, compiled
 * for the host.  hits: records as pbr_hip_query leaves them (p, p_error, n, ns, dpdu, wo and the two media
 * are read); kr: the mirror's Kr at each hit, 3 floats, textures evaluated and clamped.  followed[i]: 1 when
 * the step is taken, and rays_out + 7 * i is then the continuation (o.xyz, d.xyz, tMax = inf); else 0 and
 * seven zeros.  No context, no GPU.  PBR_E_INVALID: a NULL argument or n < 0. */
int pbr_hip_mirror_step_host(int n, const pbr_surface_hit* hits, const float* kr, float* rays_out, int32_t* followed);
/* HenyeyGreenstein::p and Sample_p (Media/Medium.h:24-27, Medium.cpp:9-26) as VolPath's shade calls
 * them: queries = g, wo.xyz, wi.xyz, u0, u1 (9 floats); out = p(wo, wi), the sampled wi.xyz and its
 * value (5 floats).  The _host form runs the same source on the CPU. */
int pbr_hip_phase_hg(pbr_hip_ctx* ctx, int n, const float* queries, float* out);
int pbr_hip_phase_hg_host(int n, const float* queries, float* out);

/* ---- The shading frame of a triangle with per-vertex normals (Shape/Triangle.cpp:148-253,
 * SurfaceInteraction::SetShadingGeometry, Core/Interaction.cpp:98-113) on caller-given triangles: the
 * function the hit path calls (csrc/pbr_shading_frame.h), compiled for the host.  No context, no GPU.
 * p and n are world space: n as the TriangleMesh constructor leaves the normals (the inverse
 * transpose applied, not renormalised).  out: 9 floats per query, n.xyz, shading.n.xyz,
 * shading.dpdu.xyz. */
typedef struct pbr_shading_query {
    float p[9];                 /* the three vertices */
    float n[9];                 /* their normals */
    float uv[6];                /* their UVs; read only when has_uv != 0 */
    float b[3];                 /* the hit's barycentrics */
    int has_uv;                 /* 0: Triangle::GetUVs' default (0,0) (1,0) (1,1) */
    int reverse_orientation;    /* the shape's own flag: flips ts */
    int swaps_handedness;       /* of the shape's transform: with the flag above, flips the geometric normal */
    int pad[2];
} pbr_shading_query;            /* 32 words */
int pbr_hip_shading_host(int n, const pbr_shading_query* queries, float* out);

/* ---- BVH construction (BVHAccel::BVHAccel, Accelerator/BVHAccel.cpp:57-87; SAH recursiveBuild
 * :97-260; flattenBVHTree :262-283) ----
 * Both builders produce the reference's node array and orderedPrims exactly (the host one is the
 * sequential algorithm; the device one, pbr_bvh_build.hip, reproduces its partitions level by level). */
enum pbr_bvh_build { PBR_BVH_BUILD_HOST = 0, PBR_BVH_BUILD_DEVICE = 1 };
/* Which builder pbr_hip_upload_scene runs (default PBR_BVH_BUILD_DEVICE). */
int pbr_hip_set_bvh_build(pbr_hip_ctx* ctx, int where);
/* The last upload's build: builder, wall ms (device: incl. the bounds upload and node download),
 * device kernel ms (0 for the host builder). */
int pbr_hip_bvh_build_info(pbr_hip_ctx* ctx, int* where, double* ms, double* kernel_ms);
/* Standalone build over n primitive world bounds (6 floats each, lo.xyz hi.xyz, prims order:
 * GeometricPrimitive::WorldBound): nodes_out has room for 2n-1 32-B LinearBVHNodes, prim_ids_out for
 * n ids; ms_out (optional, 2 doubles) = {wall ms, device kernel ms}. */
int pbr_hip_build_bvh(pbr_hip_ctx* ctx, int where, int n, const float* prim_bounds, int max_prims,
                      void* nodes_out, int* n_nodes, int32_t* prim_ids_out, double* ms_out);

/* Device build info: ABI version, gfx arch string. */
int pbr_hip_abi_version(void);
const char* pbr_hip_build_info(void);
/* The built-in Sobol' generator matrices (SobolMatrices32 layout, dims × 52 uint32, dims <= 1024):
 * the reference's SobolMatrices32; host only. */
int pbr_hip_sobol_matrices(int dims, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PBR_HIP_H */
