// variance_delivery_check.cpp — RayZath::Hip::Engine::setDenoise with HIPRZ_DENOISE_VARIANCE: the engine switches the context's variance
// estimate on (every renderWorld call is one batch) and the camera's image buffer is the variance-guided frame — hiprz_read_denoised_rgba8
// of the engine's context for sync = true, the frame of a synchronous twin one call behind for sync = false; cleared, the estimate goes
// off, accumulation restarts and the plain tone map is delivered.  Built and run by tests/test_variance_gpu.py against libhiprz_host.so.
// Prints "VARIANCE DELIVERY OK" or the first difference.
#include <cstdio>
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
static std::shared_ptr<Material> material(World& w, Color c, float metal, float rough, float emission) {
    auto m = std::make_shared<Material>();
    m->color = c, m->metalness(metal), m->roughness(rough), m->emission(emission), m->ior(1.5f);
    w.materials.push_back(m);
    return m;
}
static void instance(World& w, std::shared_ptr<Mesh> mesh, std::shared_ptr<Material> mat, vec3f pos, vec3f rot = {}, vec3f scale = {1, 1, 1}) {
    auto i = std::make_shared<Instance>();
    i->mesh = mesh, i->materials[0] = mat, i->position = pos, i->rotation = rot, i->scale = scale;
    w.instances.push_back(i);
}
static void build(World& w) {
    auto white = material(w, {230, 230, 230, 255}, 0, 1, 0), red = material(w, {200, 40, 40, 255}, 0, 1, 0);
    auto light = material(w, {255, 255, 255, 255}, 0, 1, 50);
    const float fl[4][3] = {{-2, 0, -2}, {-2, 0, 2}, {2, 0, 2}, {2, 0, -2}};
    const float bk[4][3] = {{-2, -1, 2}, {-2, 3, 2}, {2, 3, 2}, {2, -1, 2}};
    const float lf[4][3] = {{-2, -1, -2}, {-2, 3, -2}, {-2, 3, 2}, {-2, -1, 2}};
    const float lp[4][3] = {{-0.5f, 0, -0.5f}, {-0.5f, 0, 0.5f}, {0.5f, 0, 0.5f}, {0.5f, 0, -0.5f}};
    auto floor_mesh = quad(fl), cube = Mesh::generateCube();
    w.meshes = {floor_mesh, cube};
    instance(w, floor_mesh, white, {0, -1, 0});
    instance(w, quad(bk), white, {0, 0, 0});
    instance(w, quad(lf), red, {0, 0, 0});
    instance(w, quad(lp), light, {0, 2.99f, 0});
    instance(w, cube, white, {0.7f, -0.4f, -0.5f}, {0, -0.3f, 0}, {1.2f, 1.2f, 1.2f});
    w.camera.position = {0, 1, -3.5f};
    w.camera.width = 96, w.camera.height = 64;
    w.camera.focal_distance = 4.0f;
    w.camera.rayCastPixel(60, 40);
}

static bool context_image(Engine& e, bool denoised, std::vector<uint8_t>& out) {
    out.assign(size_t(96) * 64 * 4, 0);
    if (denoised) return hiprz_read_denoised_rgba8(e.context(), out.data(), out.size()) == HIPRZ_OK;
    return hiprz_tonemap(e.context()) == HIPRZ_OK && hiprz_read_rgba8(e.context(), out.data(), out.size()) == HIPRZ_OK;
}

static float batches(Engine& e) {  // the largest K of the context's estimate, -1 when it cannot be read
    std::vector<float> v(size_t(96) * 64 * 4);
    if (hiprz_read_variance(e.context(), v.data(), v.size() * sizeof(float)) != HIPRZ_OK) return -1.0f;
    float k = 0.0f;
    for (size_t i = 3; i < v.size(); i += 4) k = v[i] > k ? v[i] : k;
    return k;
}

int main() {
    try {
        World piped, synced, plain_world;
        build(piped), build(synced), build(plain_world);
        RenderConfig cfg;
        cfg.tracing.max_depth = 4, cfg.tracing.rpp = 3;
        hiprz_denoise_params params, defaults;
        hiprz_denoise_default_params(&params);
        defaults = params;
        params.flags |= HIPRZ_DENOISE_VARIANCE, params.sigma_color = 4.0f;
        Engine a(0, 1), b(0, 1), c(0, 1);
        a.setDenoise(&params), b.setDenoise(&params), c.setDenoise(&defaults);
        if (batches(c) != -1.0f) return std::printf("DIFFERENT: parameters without the flag switched the estimate on\n"), 1;
        std::vector<uint8_t> previous, image, plain;
        int compared = 0;
        for (int i = 0; i < 5; ++i) {
            a.renderWorld(piped, cfg, true, false);
            if (i > 0) {
                if (piped.camera.image_buffer != previous) return std::printf("DIFFERENT: pipelined call %d is not the synchronous twin's previous frame\n", i), 1;
                ++compared;
            }
            b.renderWorld(synced, cfg, true, true);
            c.renderWorld(plain_world, cfg, true, true);
            if (!context_image(b, true, image) || synced.camera.image_buffer != image)
                return std::printf("DIFFERENT: synchronous call %d is not hiprz_read_denoised_rgba8 of its context\n", i), 1;
            if (!context_image(b, false, plain) || plain == image) return std::printf("DIFFERENT: call %d: the denoised frame equals the plain one\n", i), 1;
            if (i > 0 && plain_world.camera.image_buffer == image) return std::printf("DIFFERENT: call %d: the flag changed nothing\n", i), 1;
            if (batches(b) != float(i + 1)) return std::printf("DIFFERENT: call %d: %g batches closed\n", i, batches(b)), 1;
            previous = synced.camera.image_buffer;
            ++compared;
        }
        a.setDenoise(nullptr), b.setDenoise(nullptr), c.setDenoise(nullptr);
        if (batches(b) != -1.0f) return std::printf("DIFFERENT: cleared, the estimate is still on\n"), 1;
        a.renderWorld(piped, cfg, true, true), b.renderWorld(synced, cfg, true, true), c.renderWorld(plain_world, cfg, true, true);
        if (!context_image(b, false, plain) || synced.camera.image_buffer != plain || piped.camera.image_buffer != plain)
            return std::printf("DIFFERENT: cleared, the engines do not deliver the plain tone map\n"), 1;
        uint32_t passes = 0, passes_plain = 0;
        if (hiprz_pass_count(b.context(), &passes) != HIPRZ_OK || hiprz_pass_count(c.context(), &passes_plain) != HIPRZ_OK || passes != 3u || passes_plain != 18u)
            return std::printf("DIFFERENT: cleared, %u passes with the flag (3: a restart), %u without (18: none)\n", passes, passes_plain), 1;
        std::printf("compared %d frames\nVARIANCE DELIVERY OK\n", compared);
    } catch (const Exception& e) {
        std::printf("Hip::Exception %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
