// frame_delivery_check.cpp — RayZath::Hip::Engine's pipelined frames (renderWorld with sync = false: hiprz_present + hiprz_read_frame of the
// previous call) against a sync = true engine one call behind, frame by frame, over two cameras of different sizes and a camera that
// moves in the middle.  Built and run by tests/test_frame_delivery_gpu.py against libhiprz_host.so.  Prints "FRAME DELIVERY OK" or the
// first difference.
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
// an open box room with a light and two boxes, seen by a 96x64 camera and a second one of 72x40
static void build(World& w) {
    auto white = material(w, {230, 230, 230, 255}, 0, 1, 0), red = material(w, {200, 40, 40, 255}, 0, 1, 0);
    auto light = material(w, {255, 255, 255, 255}, 0, 1, 50), mirror = material(w, {0xF0, 0xF0, 0xF0, 0xFF}, 0.9f, 0, 0);
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
    instance(w, cube, mirror, {-0.7f, 0.2f, 0.6f}, {0, 0.3f, 0}, {1.2f, 2.4f, 1.2f});
    instance(w, cube, white, {0.7f, -0.4f, -0.5f}, {0, -0.3f, 0}, {1.2f, 1.2f, 1.2f});
    w.camera.position = {0, 1, -3.5f};
    w.camera.width = 96, w.camera.height = 64;
    w.camera.focal_distance = 4.0f;
    w.camera.rayCastPixel(60, 40);
    auto second = std::make_shared<Camera>();
    second->position = {1.0f, 0.5f, -3.0f}, second->rotation = {0, -0.2f, 0};
    second->width = 72, second->height = 40, second->focal_distance = 3.0f;
    second->rayCastPixel(20, 30);
    w.cameras.push_back(second);
}

struct Snapshot {
    std::vector<uint8_t> image;
    std::vector<float> depth;
    uint64_t ray_count = 0;
    long instance = -2, material = -2;  // indices into the world's lists, -1: none
};
static long index_of(const World& w, const std::shared_ptr<Instance>& p) {
    for (size_t k = 0; k < w.instances.size(); ++k)
        if (w.instances[k] == p) return long(k);
    return -1;
}
static long index_of(const World& w, const std::shared_ptr<Material>& p) {
    for (size_t k = 0; k < w.materials.size(); ++k)
        if (w.materials[k] == p) return long(k);
    return -1;
}
static Snapshot snap(const World& w, const Camera& c) {
    return Snapshot{c.image_buffer, c.depth_buffer, c.ray_count, index_of(w, c.raycasted_instance), index_of(w, c.raycasted_material)};
}
static bool same(const Snapshot& a, const Snapshot& b) {
    return a.image == b.image && a.depth == b.depth && a.ray_count == b.ray_count && a.instance == b.instance && a.material == b.material;
}

int main() {
    try {
        World piped, synced;
        build(piped), build(synced);
        RenderConfig cfg;
        cfg.tracing.max_depth = 4, cfg.tracing.rpp = 3;
        Engine a(0, 1), b(0, 1);
        const int calls = 7;
        std::vector<Snapshot> previous(2);
        int compared = 0, hits = 0;
        for (int i = 0; i < calls; ++i) {
            if (i == 3)  // the first camera moves: both engines restart it
                for (World* w : {&piped, &synced}) w->camera.position = {0.3f, 1.1f, -3.4f}, w->camera.makeModified();
            a.renderWorld(piped, cfg, true, false);
            const std::vector<Camera*> pc = {&piped.camera, piped.cameras[0].get()}, sc = {&synced.camera, synced.cameras[0].get()};
            if (i == 0) {
                for (Camera* c : pc)
                    if (!c->image_buffer.empty()) return std::printf("DIFFERENT: the first pipelined call handed out a frame\n"), 1;
            } else {
                for (size_t k = 0; k < 2; ++k) {
                    const Snapshot got = snap(piped, *pc[k]);
                    if (got.image.empty() || !same(got, previous[k]))
                        return std::printf("DIFFERENT: call %d camera %zu (pixels %zu / %zu, rays %llu / %llu, instance %ld / %ld)\n", i, k,
                                           got.image.size(), previous[k].image.size(), (unsigned long long)got.ray_count,
                                           (unsigned long long)previous[k].ray_count, got.instance, previous[k].instance), 1;
                    ++compared;
                    hits += got.instance >= 0;
                }
            }
            b.renderWorld(synced, cfg, true, true);
            for (size_t k = 0; k < 2; ++k) previous[k] = snap(synced, *sc[k]);
        }
        // a sync call after pipelined ones hands out its own frame
        a.renderWorld(piped, cfg, true, true);
        b.renderWorld(synced, cfg, true, true);
        if (!same(snap(piped, piped.camera), snap(synced, synced.camera))) return std::printf("DIFFERENT: sync call after pipelined calls\n"), 1;
        std::printf("compared %d frames, %d with a ray-cast hit\n", compared, hits);
        std::printf("FRAME DELIVERY OK\n");
    } catch (const Exception& e) {
        std::printf("Hip::Exception %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
