// noise_delivery_check.cpp — RayZath::Hip::Engine::noise and ::renderUntil: the target is calibrated on the spot (half the worst tile's rms
// error of a twin engine after 8 calls), renderUntil meets it after more than 8 calls and before max_passes, its frame is the frame of a
// twin that rendered the same calls without being measured, a target of 0 ends at max_passes unmet, and noise() without the estimate is
// refused.  Built and run by tests/test_noise_gpu.py against libhiprz_host.so.  Prints "NOISE DELIVERY OK" or the first difference.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "hip_engine.hpp"

using namespace RayZath::Hip;

static std::shared_ptr<Mesh> quad(const float v[4][3]) {
    auto m = std::make_shared<Mesh>();
    for (int i = 0; i < 4; ++i) m->createVertex(v[i][0], v[i][1], v[i][2]);
    m->createTexcrd(0, 0), m->createTexcrd(0, 1), m->createTexcrd(1, 1), m->createTexcrd(1, 0);
    m->createTriangle({0, 2, 1}, {0, 2, 1});
    m->createTriangle({0, 3, 2}, {0, 3, 2});
    return m;
}
static std::shared_ptr<Material> material(World& w, Color c, float emission) {
    auto m = std::make_shared<Material>();
    m->color = c, m->metalness(0), m->roughness(1), m->emission(emission), m->ior(1.5f);
    w.materials.push_back(m);
    return m;
}
static void instance(World& w, std::shared_ptr<Mesh> mesh, std::shared_ptr<Material> mat, vec3f pos, vec3f rot = {}, vec3f scale = {1, 1, 1}) {
    auto i = std::make_shared<Instance>();
    i->mesh = mesh, i->materials[0] = mat, i->position = pos, i->rotation = rot, i->scale = scale;
    w.instances.push_back(i);
}
static void build(World& w) {
    // lit by a spot light, not by an emitter: next-event estimation brings light along every path, the regime in which the figure is
    // calibrated and falls with the passes (tests/test_noise_gpu.py: the calibration test's docstring)
    auto white = material(w, {230, 230, 230, 255}, 0), red = material(w, {200, 40, 40, 255}, 0);
    const float fl[4][3] = {{-2, 0, -2}, {-2, 0, 2}, {2, 0, 2}, {2, 0, -2}};
    const float bk[4][3] = {{-2, -1, 2}, {-2, 3, 2}, {2, 3, 2}, {2, -1, 2}};
    const float lf[4][3] = {{-2, -1, -2}, {-2, 3, -2}, {-2, 3, 2}, {-2, -1, 2}};
    auto floor_mesh = quad(fl), cube = Mesh::generateCube();
    w.meshes = {floor_mesh, cube};
    instance(w, floor_mesh, white, {0, -1, 0});
    instance(w, quad(bk), white, {0, 0, 0});
    instance(w, quad(lf), red, {0, 0, 0});
    auto lamp = std::make_shared<SpotLight>();
    lamp->position = {0.3f, 2.6f, -0.8f}, lamp->direction = {0, -1, 0.2f}, lamp->size = 0.3f, lamp->emission = 60.0f, lamp->beam_angle = 1.3f;
    w.spot_lights.push_back(lamp);
    instance(w, cube, white, {0.7f, -0.4f, -0.5f}, {0, -0.3f, 0}, {1.2f, 1.2f, 1.2f});
    w.camera.position = {0, 1, -3.5f};
    w.camera.width = 96, w.camera.height = 64;
    w.camera.focal_distance = 4.0f;
}

int main() {
    try {
        const uint32_t rpp = 4, first = 8;
        RenderConfig cfg;
        cfg.tracing.max_depth = 4, cfg.tracing.rpp = rpp;
        hiprz_noise_summary n8{}, again{};
        {
            World w;
            build(w);
            Engine plain(0, 1);
            plain.renderWorld(w, cfg);
            try {
                plain.noise(n8);
                return std::printf("DIFFERENT: noise() answered while the variance estimate is off\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: noise() without the estimate failed with %d, not HIPRZ_ERR_STATE\n", e.code), 1;
            }
        }
        World measured_world, twin_world, target_world, zero_world;
        build(measured_world), build(twin_world), build(target_world), build(zero_world);
        Engine calibration(0, 1);
        calibration.setMeasuring(true);
        for (uint32_t i = 0; i < first; ++i) calibration.renderWorld(measured_world, cfg);
        calibration.noise(n8);
        std::printf("after %u calls of %u passes: tile rms max %.6f (tile %u), rms %.6f, max %.6f, %llu of %llu pixels estimated, %llu above 1/255\n", first, rpp,
                    n8.tile_rms_max, n8.worst_tile, n8.rms, double(n8.max), (unsigned long long)n8.estimated, (unsigned long long)n8.pixels, (unsigned long long)n8.above);
        if (n8.pixels != 96u * 64u || n8.tiles_x != 3u || n8.tiles_y != 8u) return std::printf("DIFFERENT: the summary is not that of a 96 x 64 frame\n"), 1;
        if (n8.estimated != n8.pixels || !(n8.tile_rms_max > 0.0) || !(n8.rms > 0.0 && n8.rms <= n8.tile_rms_max && n8.tile_rms_max <= double(n8.max)))
            return std::printf("DIFFERENT: the figures after %u calls are not those of a noisy, fully estimated frame\n", first), 1;
        calibration.noise(again);
        if (std::memcmp(&n8, &again, sizeof n8) != 0) return std::printf("DIFFERENT: two measurements of one frame differ\n"), 1;

        const float target = float(n8.tile_rms_max / 2.0);
        const uint32_t max_passes = 16u * first * rpp;
        Engine engine(0, 1), twin(0, 1);
        const Engine::NoiseResult r = engine.renderUntil(target_world, cfg, target, max_passes);
        std::printf("renderUntil(%.6f): %u passes, tile rms max %.6f, %s\n", double(target), r.passes, r.summary.tile_rms_max, r.met ? "met" : "not met");
        if (!r.met || r.passes <= first * rpp || r.passes >= max_passes || r.passes % rpp != 0u) return std::printf("DIFFERENT: the target was not met between %u and %u passes\n", first * rpp, max_passes), 1;
        if (r.summary.estimated != r.summary.pixels || !(r.summary.tile_rms_max <= double(target))) return std::printf("DIFFERENT: met, but the rule does not hold\n"), 1;
        engine.noise(again);
        if (std::memcmp(&r.summary, &again, sizeof again) != 0) return std::printf("DIFFERENT: noise() after renderUntil is not its last measurement\n"), 1;
        twin.setMeasuring(true);
        for (uint32_t p = 0; p < r.passes; p += rpp) twin.renderWorld(twin_world, cfg);
        if (twin_world.camera.image_buffer != target_world.camera.image_buffer || twin_world.camera.depth_buffer != target_world.camera.depth_buffer ||
            twin_world.camera.ray_count != target_world.camera.ray_count)
            return std::printf("DIFFERENT: the measured engine's frame is not the frame of the same calls without measurements\n"), 1;

        Engine zero(0, 1);
        const Engine::NoiseResult z = zero.renderUntil(zero_world, cfg, 0.0f, 10u * rpp);
        if (z.met || z.passes != 10u * rpp) return std::printf("DIFFERENT: a target of 0 ended after %u passes, met %d\n", z.passes, int(z.met)), 1;
        std::printf("NOISE DELIVERY OK\n");
    } catch (const Exception& e) {
        std::printf("Hip::Exception %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
