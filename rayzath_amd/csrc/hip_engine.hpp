// hip_engine.hpp — C++ host side of the HIPGPU backend, above the C-ABI (include/hiprz.h).
//
// `RayZath::Hip::Engine` has exactly the interface the facade calls on its backends
// (RayZath/cpu_engine.hpp:17-22, RayZath/cuda_engine.cuh:34-39):
//
//     void renderWorld(World&, const RenderConfig&, bool block = true, bool sync = true);
//     std::string timingsString();
//
// The reference's host `World` cannot be compiled in this image (un-vendored Math/Graphics
// headers), so this header carries a minimal stand-alone twin of the parts of it
// the render path reads — same object kinds, member names, defaults and clamping rules
// (world.hpp:64-76, material.hpp, mesh.hpp, instance.hpp, camera.hpp, spot_light.hpp,
// direct_light.hpp, engine_parts.hpp:76-128).  INTEGRATION.md shows the adapter that fills the
// same `hiprz_scene` from the real `RayZath::Engine::World` instead.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "hiprz.h"
#include "hiprz_atlas.h"
#include "hiprz_bake.h"
#include "hiprz_gather.h"
#include "hiprz_light.h"
#include "hiprz_noise.h"
#include "hiprz_probe.h"
#include "hiprz_smooth.h"
#include "hiprz_field.h"
#include "hiprz_place.h"
#include "hiprz_view.h"
#include "hiprz_order.h"
#include "hiprz_query.h"

namespace RayZath::Hip {

// Cuda::Exception's peer (cuda_exception.hpp:9-19).  Built inside RayZath (-DHIPRZ_RAYZATH_BUILD) it derives from the
// facade's RayZath::Exception (rzexception.hpp:11-18), so the facade's `catch (RayZath::Exception&)` paths see it like a CUDA
// backend error; stand-alone (that header drags in the un-vendored CUDA driver types) it derives from the same std::runtime_error.
#ifdef HIPRZ_RAYZATH_BUILD
}  // namespace RayZath::Hip
#include "rzexception.hpp"
namespace RayZath::Hip {
using ExceptionBase = RayZath::Exception;
#else
using ExceptionBase = std::runtime_error;
#endif
struct Exception : public ExceptionBase {
    int code;
    Exception(int code_, const std::string& message) : ExceptionBase(message), code(code_) {}
};

struct vec3f {
    float x = 0, y = 0, z = 0;
};
struct Color {
    uint8_t red = 255, green = 255, blue = 255, alpha = 255;
};

// dirty-flag base, after Updatable/StateRegister (updatable.cpp:23-51)
class Updatable {
public:
    bool isModified() const { return m_modified; }
    void makeModified() { m_modified = true; }
    void makeUnmodified() { m_modified = false; }

private:
    bool m_modified = true;
};

struct TextureBuffer {  // render_parts.hpp:113-222
    uint32_t kind = HIPRZ_TEX_RGBA8, width = 0, height = 0;
    std::vector<uint8_t> bitmap;  // row-major, top row first
    float scale[2] = {1, 1}, rotation = 0, translation[2] = {0, 0};
    uint32_t sampling = HIPRZ_TEX_FILTER_POINT | HIPRZ_TEX_ADDRESS_WRAP;  // "filter mode" / "address mode" of the scene file: CUDA-compat mode only
};

struct Material {  // material.hpp:119-160; setters clamp as material.cpp:32-61
    Color color{0xC0, 0xC0, 0xC0, 0xFF};
    std::shared_ptr<TextureBuffer> texture, normal_map, metalness_map, roughness_map, emission_map;
    void metalness(float v) { m_metalness = v < 0 ? 0 : v > 1 ? 1 : v; }
    void roughness(float v) { m_roughness = v < 0 ? 0 : v > 1 ? 1 : v; }
    void emission(float v) { m_emission = v < 0 ? 0 : v; }
    void ior(float v) { m_ior = v < 1 ? 1 : v; }
    void scattering(float v) { m_scattering = v < 0 ? 0 : v; }
    float metalness() const { return m_metalness; }
    float roughness() const { return m_roughness; }
    float emission() const { return m_emission; }
    float ior() const { return m_ior; }
    float scattering() const { return m_scattering; }

private:
    float m_metalness = 0, m_roughness = 0, m_emission = 0, m_ior = 1.5f, m_scattering = 0;
};

struct Mesh {  // mesh.hpp
    static constexpr uint32_t ids_unused = 0xFFFFFFFFu;
    std::vector<float> vertices, texcrds, normals;                // xyz / uv / xyz
    std::vector<uint32_t> tri_vertices, tri_texcrds, tri_normals; // 3 per triangle
    std::vector<uint32_t> tri_materials;                          // 1 per triangle
    uint32_t createVertex(float x, float y, float z);
    uint32_t createTexcrd(float u, float v);
    uint32_t createTriangle(std::array<uint32_t, 3> vs, std::array<uint32_t, 3> ts = {ids_unused, ids_unused, ids_unused},
                            std::array<uint32_t, 3> ns = {ids_unused, ids_unused, ids_unused}, uint32_t material_id = 0);
    static std::shared_ptr<Mesh> generateCube();  // world.cpp:129-166
};

struct Group {  // group.hpp: a transformation over instances and sub-groups (groupable.hpp)
    vec3f position, rotation, scale{1, 1, 1};
    std::shared_ptr<Group> group;  // the group this one belongs to
};

struct Instance {  // instance.hpp:9-60
    static constexpr uint32_t materialCapacity() { return 64; }
    vec3f position, rotation, scale{1, 1, 1};
    std::shared_ptr<Mesh> mesh;
    std::array<std::shared_ptr<Material>, 64> materials;
    std::shared_ptr<Group> group;  // Groupable::group()
};

struct SpotLight {  // spot_light.hpp
    vec3f position, direction{0, -1, 0};
    Color color;
    float size = 0.5f, emission = 100.0f, beam_angle = 1.0f;
};
struct DirectLight {  // direct_light.hpp
    vec3f direction{0, -1, 0};
    Color color;
    float emission = 100.0f, angular_size = 0.1f;
};

struct Camera : public Updatable {  // camera.hpp:127-161
    vec3f position{0, 0, -10}, rotation;
    uint32_t width = 1280, height = 720;
    float fov = 1.57079632679f, near_plane = 1.0e-2f, far_plane = 1.0e3f;
    float focal_distance = 10.0f, aperture = 0.02f, exposure_time = 1.0f / 60.0f;
    float temporal_blend = 0.75f;  // camera.hpp:135; read with HIPRZ_COMPAT_REPROJECTION only
    bool enabled = true;  // camera.hpp:150; disabled cameras are skipped by the renderers (cpu_engine_renderer.cpp:99)
    // outputs the backend writes (camera.hpp:50-56, 113-119)
    std::vector<uint8_t> image_buffer;  // RGBA8 W*H
    std::vector<float> depth_buffer;    // W*H
    uint64_t ray_count = 0;
    // Kernel::rayCast (cpu_engine_kernel.cpp:102-111): after every frame, what the ray through this pixel meets — the editor's picking
    void rayCastPixel(uint32_t x, uint32_t y) {  // camera.cpp:159-165: clamped, marks the camera modified (accumulation goes on: the record the
                                                 // backend mirrors is unchanged, and neither reference engine restarts for MakeModified alone)
        ray_cast_pixel[0] = x >= width ? width - 1 : x, ray_cast_pixel[1] = y >= height ? height - 1 : y;
        makeModified();
    }
    uint32_t ray_cast_pixel[2] = {0, 0};
    std::shared_ptr<Instance> raycasted_instance;  // camera.hpp:55-56 (m_raycasted_instance / m_raycasted_material)
    std::shared_ptr<Material> raycasted_material;
};

struct World : public Updatable {  // world.hpp:64-76
    World();
    std::vector<std::shared_ptr<Material>> materials;
    std::vector<std::shared_ptr<Mesh>> meshes;
    std::vector<std::shared_ptr<Instance>> instances;
    std::vector<std::shared_ptr<SpotLight>> spot_lights;
    std::vector<std::shared_ptr<DirectLight>> direct_lights;
    Camera camera;                                  // the first camera ...
    std::vector<std::shared_ptr<Camera>> cameras;   // ... and the others: every enabled one is rendered per call (cpu_engine_renderer.cpp:97-117)
    std::vector<std::shared_ptr<Group>> groups;
    Material material;          // world / sky medium (world.cpp:33-38)
    Material default_material;  // world.cpp:39-43
    // How an instance inside groups is mirrored.  Cpu (default): what the CPU engine does — the bounding box comes from the
    // transformation composed through its groups (Instance::calculateBoundingBox, instance.cpp:125-155) while rays are taken into
    // the instance's OWN transformation (cpu_engine_kernel.cpp:308); the two agree only outside groups.  Cuda: the composed
    // transformation for both (cuda_instance.cu:244, transformationInGroup()).
    enum class GroupTransforms { Cpu, Cuda } group_transforms = GroupTransforms::Cpu;
    // materials / lights changed but no geometry: the engine replaces those records only (updatable.cpp:23-51 per container)
    void makeShadingModified() { m_shading_modified = true; }
    bool isShadingModified() const { return m_shading_modified; }
    void makeShadingUnmodified() { m_shading_modified = false; }
    // vertices of meshes and / or transformations of instances moved; the same meshes with the same triangles in the same instances
    // (an animation frame).  Where the context holds device-built trees the engine then refits them on the device and rebuilds the
    // world tree there (hiprz_update_triangles / hiprz_update_instances) instead of building every tree again on the host, as the
    // reference does at any change (component_container.hpp:259-363); otherwise it is an ordinary modification.
    void makeMoved() { m_moved = true; }
    bool isMoved() const { return m_moved; }
    void makeUnmoved() { m_moved = false; }

private:
    bool m_shading_modified = false, m_moved = false;
};

struct LightSampling {  // engine_parts.hpp:76-94
    uint8_t spot_light = 1, direct_light = 1;
};
struct Tracing {  // engine_parts.hpp:95-113
    uint8_t max_depth = 16;
    uint32_t rpp = 8;
};
struct RenderConfig {
    LightSampling light_sampling;
    Tracing tracing;
    uint32_t seed = 20240501u;
};

// The flattened snapshot with owning storage (what hiprz_upload_scene copies).
struct FlatScene {
    std::vector<hiprz_node> nodes;
    std::vector<uint32_t> tlas_order;
    std::vector<hiprz_tri> tris;
    std::vector<hiprz_tri_attr> tri_attrs;
    std::vector<hiprz_instance> instances;
    std::vector<int32_t> inst_materials;
    std::vector<hiprz_material> materials;
    std::vector<hiprz_texture> textures;
    std::vector<uint8_t> texels;
    std::vector<hiprz_spot_light> spot_lights;
    std::vector<hiprz_direct_light> direct_lights;
    std::vector<const void*> maps;  // the map objects behind `textures`, by identity, in texture-index order (host-side bookkeeping only)
    hiprz_scene view() const;
};
FlatScene flatten(const World& world);           // pure host
FlatScene flattenShading(const World& world);    // materials + lights only (for hiprz_update_shading): pure host
// triangles + instances only (for hiprz_update_triangles / hiprz_update_instances): the meshes' triangles in the order of an earlier
// flatten() (`uploaded_sources` = its tris[k].source_index), no tree is built.  Empty when the world no longer matches that order.
FlatScene flattenMotion(const World& world, const std::vector<uint32_t>& uploaded_sources);
hiprz_camera cameraRecord(const Camera& camera); // pure host

class Engine {
public:
    // throws Hip::Exception: the facade then falls back to CPU (rayzath.cpp:21-28).  `streams`: how many contexts-with-a-stream share
    // the GPU (hiprz_create_multi with the device named that often: one share's sorts, bookkeeping and kernel tails run beside another
    // share's walks); 0 = chosen when the first world is rendered — two for a world without lights, one otherwise (defaultStreams).
    explicit Engine(int device = 0, int streams = 0);
    explicit Engine(const std::vector<int>& devices);  // one context over several GPUs: tiles interleaved, peer-to-peer gather
    static int defaultStreams(const World& world) { return world.spot_lights.empty() && world.direct_lights.empty() ? 2 : 1; }
    void mode(uint32_t compat_flags);  // hiprz_set_mode: behaviours of the CUDA engine (default 0 = the CPU kernel)
    void tree(uint32_t tree);          // hiprz_set_tree, applied at the next scene upload
    // How the devices of Engine(devices) divide a frame (hiprz_set_shard_mode; no counterpart in the reference, which drives one device:
    // cuda_engine_core.cu:17).  Tiles (default): interleaved 32x8 tiles — the one-device frame bit for bit, a frame of `rpp` passes arrives
    // sooner: what an interactive host wants.  Samples: every device renders the whole frame on its own seed stream and the accumulators are
    // summed — a renderWorld call adds devices * rpp samples per pixel and rayCount() grows by as many rays; aggregate rays per second scale
    // with the devices where tile sharding is held back by its slowest tile: what a converging (headless / offline) host
    // wants — hiprz_headless --devices picks it.  Restarts accumulation.
    enum class ShardMode : uint32_t { Tiles = HIPRZ_SHARD_TILES, Samples = HIPRZ_SHARD_SAMPLES };
    void shardMode(ShardMode mode);
    // hiprz_set_denoise: while set, the cameras' image buffers receive the frame filtered by the edge-avoiding a-trous filter over the
    // first-hit guides (include/hiprz.h), for sync true and false alike; nullptr clears it (the default).  Depth buffers stay as they are.
    // Parameters with HIPRZ_DENOISE_VARIANCE also switch the context's variance estimate on (hiprz_set_variance; every renderWorld call is
    // one batch), any others switch it off: a change of that restarts accumulation.
    void setDenoise(const hiprz_denoise_params* params);
    // The noise level of the first camera's frame (include/hiprz_noise.h): the standard error of the displayed luminance per 32x8 tile,
    // summarised; a pixel has an estimate once `min_batches` renderWorld calls closed a batch for it.  Needs the variance estimate
    // (renderUntil or setDenoise with HIPRZ_DENOISE_VARIANCE switched it on): HIPRZ_ERR_STATE otherwise.  Waits for the stream; changes no frame.
    void noise(hiprz_noise_summary& out, float threshold = 1.0f / 255.0f, uint32_t min_batches = 8);
    // Ray queries (include/hiprz_query.h): the closest hit / the occlusion of every ray of `rays` in the world of the last renderWorld call,
    // in caller order; normalize: the device's normalized() is applied to the directions first.  Wait for the stream; change no frame.
    // ordered: walked in the renderer's sorted ray order (include/hiprz_order.h) — the same bytes, sooner for a large batch of rays in no
    // particular order, later for rays that arrive coherent.
    std::vector<hiprz_hit> castRays(const std::vector<hiprz_ray>& rays, bool normalize = false, bool ordered = false);
    std::vector<uint32_t> occluded(const std::vector<hiprz_ray>& rays, bool normalize = false, bool ordered = false);
    // Occlusion baking (include/hiprz_bake.h): per surface point of `points`, how many of K rays of the cosine table (K, S) are occluded in
    // the world of the last renderWorld call and the sum of the directions that are not; the rays are made and counted on the device.
    // Waits for the stream; changes no frame.
    std::vector<hiprz_bake_texel> bakeOcclusion(const std::vector<hiprz_bake_point>& points, uint32_t K = 64, uint32_t S = 4, uint32_t seed = 0);
    // Bake atlases (include/hiprz_atlas.h): the charts of `parts` — triangles with positions and normals in the mesh's own space and UVs in
    // atlas units, placed as instance `instance` of the world of the last renderWorld call is now, ids numbered through the list — are
    // rasterised on the device into one surface point per texel of a width x height atlas, the points are baked as bakeOcclusion bakes
    // them without visiting the host, and the texels are dilated by `rings` rings into the gutters.  Texel (x, y) is entry y * width + x;
    // ring: 0 covered, r filled in ring r, HIPRZ_ATLAS_NONE still empty.  Waits for the stream; changes no frame.
    struct AtlasPart {
        uint32_t instance;
        std::vector<hiprz_atlas_tri> charts;
    };
    struct BakedAtlas {
        uint32_t width = 0, height = 0;
        std::vector<hiprz_bake_texel> texels;
        std::vector<hiprz_atlas_sample> samples;
        std::vector<uint32_t> ring;
    };
    BakedAtlas bakeAtlas(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, uint32_t K = 64, uint32_t S = 4, uint32_t seed = 0, uint32_t rings = 2,
                         float near_ = 1.0e-3f, float far_ = 3.0e38f);
    // Light baking (include/hiprz_light.h): per surface point of `points`, the direct light of the spot and direct lights of the world of the
    // last renderWorld call with their shadows, K shadow rays per light from the disk table (K, S); `range` selects a sub-range of the
    // lights (nullptr: all of them; one call per range gives per-light maps).  Waits for the stream; changes no frame.
    std::vector<hiprz_light_texel> bakeLight(const std::vector<hiprz_bake_point>& points, uint32_t K = 16, uint32_t S = 4, uint32_t seed = 0,
                                             const hiprz_light_range* range = nullptr);
    // bakeAtlas with bakeLight's quantity per texel: atlas points, the light bake where they lie on the device, `rings` rings of dilation.
    // smooth: nullptr, or the params of smoothTexels, run on the device between the bake and the dilation.
    struct LitAtlas {
        uint32_t width = 0, height = 0;
        std::vector<hiprz_light_texel> texels;
        std::vector<hiprz_atlas_sample> samples;
        std::vector<uint32_t> ring;
    };
    LitAtlas bakeLightAtlas(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, uint32_t K = 16, uint32_t S = 4, uint32_t seed = 0, uint32_t rings = 2,
                            float near_ = 1.0e-3f, float far_ = 3.0e38f, const hiprz_light_range* range = nullptr, const hiprz_smooth_params* smooth = nullptr);
    // Bounce baking (include/hiprz_gather.h): per surface point of `points`, the mean over the K hemisphere rays of the cosine table (K, S) of
    // what the width x height atlas `source` (16-byte records: RGB and a word, HIPRZ_GATHER_INVALID where a texel has no value) holds under
    // each ray's closest hit in the world of the last renderWorld call; `sky` (three floats, nullptr: 0) for a ray that hits nothing.  The
    // chart map says where a hit lies in the atlas: chartMap(parts, n) for the parts of an atlas over a world of n instances.  Waits for the
    // stream; changes no frame.
    struct Record {  // a source, albedo or emission texel
        float rgb[3];
        uint32_t word;
    };
    struct ChartMap {
        std::vector<uint32_t> base;  // per instance: the id of its first chart, HIPRZ_GATHER_NONE for one that is in no part
        std::vector<hiprz_gather_chart> uv;
    };
    static ChartMap chartMap(const std::vector<AtlasPart>& parts, uint32_t n_instances);
    std::vector<hiprz_gather_texel> gather(const std::vector<hiprz_bake_point>& points, const std::vector<Record>& source, uint32_t width, uint32_t height,
                                           const ChartMap& charts, uint32_t K = 64, uint32_t S = 4, uint32_t seed = 0, const float* sky = nullptr);
    // Probe baking (include/hiprz_probe.h): per probe of `probes` — a point of free space, its `normal` the axis of its frame — nine
    // spherical-harmonic coefficients per colour of the light arriving from all directions: the K rays of the sphere table (K, S) read the
    // width x height atlas `source` through `charts` by the rule of gather, and, with `direct`, the lights of the world of the last
    // renderWorld call are added with their shadows from the disk table (light_K, light_S), on the device, on top of the gathered records.
    // The bytes of Context.bake_probes.  Waits for the stream; changes no frame.
    std::vector<hiprz_probe_sh> bakeProbes(const std::vector<hiprz_bake_point>& probes, const std::vector<Record>& source, uint32_t width, uint32_t height,
                                           const ChartMap& charts, uint32_t K = 64, uint32_t S = 4, uint32_t light_K = 16, uint32_t light_S = 4, uint32_t seed = 0,
                                           const float* sky = nullptr, const hiprz_light_range* range = nullptr, bool direct = true);
    // E(n) of one record for the unit normal n (hiprz_probe_irradiance): what a lightmap texel with that normal would hold at the probe
    static std::array<float, 3> probeIrradiance(const hiprz_probe_sh& sh, const float n[3]);
    // bakeLightAtlas and then `bounces` radiosity steps: the source albedo * (direct + indirect) + emission per texel (emission may be
    // empty: 0), `rings` rings of dilation, and the gather at the atlas's points.  `direct` and `indirect` come back dilated, with the ring
    // map of bakeLightAtlas.  This host has no device allocator of its own: the steps go through the libraries' host-pointer calls, and
    // give the bytes of Context.bake_bounce_atlas, which keeps everything on the device.  smooth: nullptr, or the params of smoothTexels:
    // direct is smoothed once right after its bake and every bounce's indirect right after its gather.
    struct BouncedAtlas {
        uint32_t width = 0, height = 0;
        std::vector<hiprz_light_texel> direct;
        std::vector<hiprz_gather_texel> indirect;
        std::vector<uint32_t> ring;
    };
    BouncedAtlas bakeBounceAtlas(const std::vector<AtlasPart>& parts, uint32_t n_instances, uint32_t width, uint32_t height, const std::vector<Record>& albedo,
                                 const std::vector<Record>& emission, uint32_t bounces = 1, uint32_t K = 64, uint32_t S = 4, uint32_t light_K = 16, uint32_t light_S = 4,
                                 uint32_t seed = 0, uint32_t rings = 2, const float* sky = nullptr, float near_ = 1.0e-3f, float far_ = 3.0e38f,
                                 const hiprz_smooth_params* smooth = nullptr);
    // Lightmap smoothing (include/hiprz_smooth.h): the width x height records of an atlas (RGB and a word: light or gather texels)
    // smoothed along its surfaces under the guidance of the atlas's points, by an a-trous filter of params.iterations steps that never
    // blends a texel with a neighbour of the atlas that is not its neighbour on the surface.  A texel without a value keeps its 16 bytes;
    // every word comes back unchanged.  The bytes of Context.smooth_texels.  Waits for the stream; changes no frame.
    std::vector<Record> smoothTexels(const std::vector<hiprz_bake_point>& points, const std::vector<Record>& records, uint32_t width, uint32_t height,
                                     const hiprz_smooth_params& params);
    // Probe fields (include/hiprz_field.h).  bakeVisibility: per probe an 8 x 8 octahedral map of the mean and the mean square of
    // min(distance to the closest hit, reach) over the K rays of the sphere table (K, S), K >= 64, in the world of the last renderWorld
    // call.  lookupField: the irradiance the probes of `grid` (their positions `probes`, records `sh` and — unless empty — visibility
    // records `vis`, in the grid's C order) give every point of `points`, evaluated on the device; with `vis` a probe behind a wall does
    // not leak.  The bytes of Context.bake_visibility and Context.lookup_field.  Wait for the stream; change no frame.
    std::vector<hiprz_field_vis> bakeVisibility(const std::vector<hiprz_bake_point>& probes, float reach, uint32_t K = 256, uint32_t S = 4, uint32_t seed = 0);
    std::vector<hiprz_field_result> lookupField(const hiprz_field_grid& grid, const std::vector<hiprz_bake_point>& probes, const std::vector<hiprz_probe_sh>& sh,
                                                const std::vector<hiprz_field_vis>& vis, const std::vector<hiprz_bake_point>& points,
                                                const hiprz_field_params& params = hiprz_field_params{0.0f, 0u, {0u, 0u}});
    // Probe placement (include/hiprz_place.h): the probes moved out of geometry and away from the surface they hug, by the rays of the
    // sphere table (K, S), K >= 64, in the world of the last renderWorld call; at most params.iterations moves, the offset within
    // params.max_offset on every axis.  The moved probes, and in `records` (unless null) the offset, the state at the final position, the
    // moves made and what the probe sees there.  The bytes of Context.place_probes.  Waits for the stream; changes no frame.
    std::vector<hiprz_bake_point> placeProbes(const std::vector<hiprz_bake_point>& probes, const hiprz_place_params& params, std::vector<hiprz_place_record>* records = nullptr,
                                              uint32_t K = 256, uint32_t S = 4, uint32_t seed = 0);
    // Baked view (include/hiprz_view.h): the frame of the selected camera of the last renderWorld call, shaded from the width x height atlas
    // `source` (what a texel sends on: albedo x (direct + indirect) + emission, composed and dilated) through `charts` and — for objects
    // outside the atlas, unless `field` is null — from a probe field (lookupField's arguments, as host pointers) times the surface's colour.
    // One 16-byte record per pixel, row-major: the RGB and kind << 28 | count; with `image` also the float4 (r, g, b, 1) per pixel.  The
    // bytes of Context.view.  Waits for the stream; changes no frame.
    std::vector<hiprz_view_pixel> bakedView(const std::vector<Record>& source, uint32_t width, uint32_t height, const ChartMap& charts, const hiprz_view_field* field = nullptr,
                                            const float* sky = nullptr, uint32_t filter = HIPRZ_VIEW_NEAREST, std::vector<float>* image = nullptr);
    // The variance estimate on for noise() whatever setDenoise asks for (renderUntil sets it); a real change restarts accumulation.
    void setMeasuring(bool enabled);
    // Render to a noise target: renderWorld(sync = true) calls, each one batch of tracing.rpp passes, until EVERY pixel of the frame has an
    // estimate and summary.tile_rms_max <= target (display units), or until max_passes passes were rendered; measured after every call from
    // the min_batches-th on.  tile_rms_max, not rms: noise concentrated in one region is not averaged away by a clean background.
    // Switches the variance estimate on if it was off — a real change, which restarts accumulation — and leaves it on.
    struct NoiseResult {
        hiprz_noise_summary summary;  // the last measurement
        uint32_t passes;              // rendered by this call
        bool met;
    };
    NoiseResult renderUntil(World& world, const RenderConfig& render_config, float target, uint32_t max_passes, uint32_t min_batches = 8);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    // `block` is accepted and ignored like in both reference backends.  sync = true: the camera buffers hold
    // THIS call's frame on return.  sync = false: the call only enqueues; the buffers are filled by the next call
    // (the CUDA backend's pipelined readback, cuda_engine_core.cu:115-120).  A device error met after a
    // non-sync call returned is stored and thrown by the next call (cuda_engine_core.cu:41).
    void renderWorld(World& world, const RenderConfig& render_config, bool block = true, bool sync = true);
    std::string timingsString();

    hiprz_ctx* context() {  // for tests: settles the stream count as it is
        m_streams_pending = false;
        return m_ctx;
    }

private:
    void check(int rc);
    // camera `camera` gets frame `sequence` of the selected camera of the context (hiprz_read_frame: waits for that frame's copy only)
    void deliver(Camera& camera, const World& world, uint32_t sequence);
    std::vector<Camera*> enabledCameras(World& world) const;

    hiprz_ctx* m_ctx = nullptr;
    int m_device = 0;
    bool m_streams_pending = false;  // the context is still the single one of the constructor: the first world decides
    uint32_t m_mode = 0, m_tree = HIPRZ_TREE_AUTO;  // what mode() / tree() set (the hosts' default trees: per scene), for the context that replaces it
    bool m_denoise = false;
    hiprz_denoise_params m_denoise_params{};
    bool m_measuring = false;               // renderUntil was called: the variance estimate stays on for its measurements
    hiprz_noise_meter* m_meter = nullptr;   // on the head device, created at the first measurement
    hiprz_query* m_query = nullptr;         // bound to m_ctx, created at the first query
    hiprz_query* query();
    hiprz_order* m_order = nullptr;         // bound to m_ctx, created at the first ordered query
    hiprz_order* order();
    hiprz_bake* m_bake = nullptr;           // bound to m_ctx, created at the first bake; it holds the cosine table of (m_bake_k, m_bake_s)
    uint32_t m_bake_k = 0, m_bake_s = 0;
    hiprz_bake* baker(uint32_t K, uint32_t S);  // m_bake holding the cosine table of (K, S)
    hiprz_atlas* m_atlas = nullptr;         // bound to m_ctx, created at the first bakeAtlas
    hiprz_atlas* atlasWith(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, float near_, float far_, const char* what);  // m_atlas holding the points of `parts` (not empty: the callers refuse that)
    hiprz_light* m_light = nullptr;         // bound to m_ctx, created at the first light bake; it holds the disk table of (m_light_k, m_light_s)
    uint32_t m_light_k = 0, m_light_s = 0;
    hiprz_light* lighter(uint32_t K, uint32_t S);  // m_light holding the disk table of (K, S)
    hiprz_smooth* m_smooth = nullptr;       // bound to m_ctx, created at the first smoothing
    hiprz_smooth* smoother();               // m_smooth, created when there is none
    hiprz_field* m_field = nullptr;         // bound to m_ctx, created at the first bakeVisibility or lookupField; it holds the sphere table of (m_field_k, m_field_s)
    uint32_t m_field_k = 0, m_field_s = 0;
    hiprz_field* fielder();                 // m_field, created when there is none
    hiprz_place* m_place = nullptr;         // bound to m_ctx, created at the first placeProbes; it holds the sphere table of (m_place_k, m_place_s)
    uint32_t m_place_k = 0, m_place_s = 0;
    hiprz_view* m_view = nullptr;           // bound to m_ctx, created at the first bakedView
    hiprz_probe* m_probe = nullptr;         // bound to m_ctx, created at the first bakeProbes; it holds the sphere table of (m_probe_k, m_probe_s) and the disk table
    uint32_t m_probe_k = 0, m_probe_s = 0, m_probe_light_k = 0, m_probe_light_s = 0;
    hiprz_gather* m_gather = nullptr;       // bound to m_ctx, created at the first gather; it holds the cosine table of (m_gather_k, m_gather_s)
    uint32_t m_gather_k = 0, m_gather_s = 0;
    hiprz_gather* gatherer(uint32_t K, uint32_t S, const ChartMap& charts);  // m_gather holding the cosine table of (K, S) and `charts`
    int wantVariance() const { return m_measuring || (m_denoise && (m_denoise_params.flags & HIPRZ_DENOISE_VARIANCE)) ? 1 : 0; }
    std::mutex m_mutex;  // renderWorld is serialised (cpu_engine_core.cpp:15)
    bool m_pending_readback = false;
    struct PendingFrame {  // a frame a non-sync call presented: the next call hands it out once its own renders are enqueued
        size_t slot;
        Camera* camera;
        uint32_t sequence;
    };
    std::vector<PendingFrame> m_pending_frames;
    std::vector<uint32_t> m_presented;                           // camera k of the context: sequence of its newest hiprz_present
    std::vector<std::pair<uint32_t, uint32_t>> m_frame_sizes;   // ... and the size of its frame slots (an upload at another size restarts the sequence)
    std::unique_ptr<Exception> m_deferred;
    const World* m_last_world = nullptr;
    std::vector<const Camera*> m_camera_slots;  // camera k of the context mirrors this camera
    std::vector<hiprz_camera> m_camera_records; // ... as this record (a modified camera whose record is unchanged is not uploaded again)
    std::vector<const void*> m_uploaded_maps;   // the maps of the uploaded scene: hiprz_update_shading may only refer to these, by these indices
    std::vector<uint32_t> m_uploaded_sources;   // source_index of every uploaded triangle, in upload order (World::makeMoved: the order new vertices go up in)
    size_t m_uploaded_instances = 0;
    uint32_t m_moved_frames = 0;                // consecutive frames that went through the refit (World::makeMoved)
    static constexpr uint32_t kRebuildEvery = 16u;
};

}  // namespace RayZath::Hip
