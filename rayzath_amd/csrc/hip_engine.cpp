// hip_engine.cpp — see hip_engine.hpp.  Host-only C++ (no device code): everything below the
// C-ABI lives in hiprz_api.hip / hiprz_scene.hip / hiprz_readback.hip / hiprz_host.cpp / hiprz_scene_host.cpp.
#include "hip_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>

namespace RayZath::Hip {

// ---- Mesh ----
uint32_t Mesh::createVertex(float x, float y, float z) {
    vertices.insert(vertices.end(), {x, y, z});
    return uint32_t(vertices.size() / 3 - 1);
}
uint32_t Mesh::createTexcrd(float u, float v) {
    texcrds.insert(texcrds.end(), {u, v});
    return uint32_t(texcrds.size() / 2 - 1);
}
uint32_t Mesh::createTriangle(std::array<uint32_t, 3> vs, std::array<uint32_t, 3> ts, std::array<uint32_t, 3> ns,
                              uint32_t material_id) {
    tri_vertices.insert(tri_vertices.end(), vs.begin(), vs.end());
    tri_texcrds.insert(tri_texcrds.end(), ts.begin(), ts.end());
    tri_normals.insert(tri_normals.end(), ns.begin(), ns.end());
    tri_materials.push_back(material_id);
    return uint32_t(tri_materials.size() - 1);
}
std::shared_ptr<Mesh> Mesh::generateCube() {  // world.cpp:129-166
    auto m = std::make_shared<Mesh>();
    const float v[8][3] = {{-.5f, .5f, -.5f}, {-.5f, .5f, .5f}, {.5f, .5f, .5f}, {.5f, .5f, -.5f},
                           {-.5f, -.5f, -.5f}, {-.5f, -.5f, .5f}, {.5f, -.5f, .5f}, {.5f, -.5f, -.5f}};
    for (auto& p : v) m->createVertex(p[0], p[1], p[2]);
    m->createTexcrd(0, 0), m->createTexcrd(0, 1), m->createTexcrd(1, 1), m->createTexcrd(1, 0);
    const uint32_t t[12][3] = {{1, 2, 0}, {3, 0, 2}, {4, 7, 5}, {6, 5, 7}, {0, 3, 4}, {7, 4, 3},
                               {2, 1, 6}, {5, 6, 1}, {3, 2, 7}, {6, 7, 2}, {1, 0, 5}, {4, 5, 0}};
    for (int i = 0; i < 12; ++i)
        m->createTriangle({t[i][0], t[i][1], t[i][2]}, i % 2 == 0 ? std::array<uint32_t, 3>{1, 2, 0} : std::array<uint32_t, 3>{3, 0, 2});
    return m;
}

World::World() {
    material.color = Color{0xFF, 0xFF, 0xFF, 0x00};  // world.cpp:33-38
    material.ior(1.0f);
    default_material.color = Color{0xC0, 0xC0, 0xC0, 0xFF};  // Palette::LightGrey (value assumed)
}

// ---- flattening ----
hiprz_scene FlatScene::view() const {
    hiprz_scene s{};
    s.n_nodes = uint32_t(nodes.size()), s.nodes = nodes.data();
    s.tlas_root = 0;
    s.n_tlas_order = uint32_t(tlas_order.size()), s.tlas_order = tlas_order.data();
    s.n_tris = uint32_t(tris.size()), s.tris = tris.data(), s.tri_attrs = tri_attrs.data();
    s.n_instances = uint32_t(instances.size()), s.instances = instances.data();
    s.n_inst_materials = uint32_t(inst_materials.size()), s.inst_materials = inst_materials.data();
    s.n_materials = uint32_t(materials.size()), s.materials = materials.data();
    s.n_textures = uint32_t(textures.size()), s.textures = textures.data();
    s.texel_bytes = texels.size(), s.texels = texels.data();
    s.n_spot_lights = uint32_t(spot_lights.size()), s.spot_lights = spot_lights.data();
    s.n_direct_lights = uint32_t(direct_lights.size()), s.direct_lights = direct_lights.data();
    return s;
}

namespace {
void put3(float* dst, const vec3f& v) { dst[0] = v.x, dst[1] = v.y, dst[2] = v.z; }
void normalize3(float* v) {
    const float s = 1.0f / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] *= s, v[1] *= s, v[2] *= s;
}
}  // namespace

namespace {
// Transformation (render_parts.hpp:39-69) of an instance, composed through its groups as Transformation::operator*= does
// (render_parts.cpp:75-82): position rotated by the group's axes and moved by its position, axes rotated, scales multiplied.
struct Xform {
    float p[3], s[3], x[3], y[3], z[3];
};
void forward(const Xform& g, float* v) {  // CoordSystem::transformForward: x_axis * v.x + y_axis * v.y + z_axis * v.z
    const float a = v[0], b = v[1], c = v[2];
    for (int k = 0; k < 3; ++k) v[k] = (g.x[k] * a + g.y[k] * b) + g.z[k] * c;
}
Xform own_transform(const vec3f& position, const vec3f& rotation, const vec3f& scale) {
    Xform t;
    put3(t.p, position), put3(t.s, scale);
    float rot[3];
    put3(rot, rotation);
    hiprz_axes_from_rotation(rot, t.x, t.y, t.z);
    return t;
}
Xform in_group(const Instance& inst) {  // Instance::calculateBoundingBox, instance.cpp:125-133
    Xform t = own_transform(inst.position, inst.rotation, inst.scale);
    for (const Group* g = inst.group.get(); g; g = g->group.get()) {
        const Xform gt = own_transform(g->position, g->rotation, g->scale);
        forward(gt, t.p);
        for (int k = 0; k < 3; ++k) t.p[k] += gt.p[k];
        forward(gt, t.x), forward(gt, t.y), forward(gt, t.z);
        for (int k = 0; k < 3; ++k) t.s[k] *= gt.s[k];
    }
    return t;
}
void store(hiprz_instance& r, const Xform& t) {
    std::memcpy(r.position, t.p, 12), std::memcpy(r.scale, t.s, 12);
    std::memcpy(r.x_axis, t.x, 12), std::memcpy(r.y_axis, t.y, 12), std::memcpy(r.z_axis, t.z, 12);
}
void flatten_lights(const World& world, FlatScene& f) {
    for (const auto& l : world.spot_lights) {
        hiprz_spot_light r{};
        put3(r.position, l->position), put3(r.direction, l->direction);
        normalize3(r.direction);
        r.size = std::max(l->size, std::numeric_limits<float>::min()), r.emission = std::max(l->emission, 0.0f);
        r.color[0] = l->color.red, r.color[1] = l->color.green, r.color[2] = l->color.blue, r.color[3] = l->color.alpha;
        r.angle = std::min(std::max(l->beam_angle, 0.0f), 3.14159f), r.cos_angle = std::cos(r.angle);
        f.spot_lights.push_back(r);
    }
    for (const auto& l : world.direct_lights) {
        hiprz_direct_light r{};
        put3(r.direction, l->direction);
        normalize3(r.direction);
        r.emission = std::max(l->emission, 0.0f);
        r.color[0] = l->color.red, r.color[1] = l->color.green, r.color[2] = l->color.blue, r.color[3] = l->color.alpha;
        r.angular_size = std::min(std::max(l->angular_size, 0.0f), 3.14159265358979f), r.cos_angular_size = std::cos(r.angular_size);
        f.direct_lights.push_back(r);
    }
}
}  // namespace

FlatScene flatten(const World& world) {
    FlatScene f;
    std::map<const TextureBuffer*, int32_t> tex_index;
    auto tex_id = [&](const std::shared_ptr<TextureBuffer>& t) -> int32_t {
        if (!t) return -1;
        auto it = tex_index.find(t.get());
        if (it != tex_index.end()) return it->second;
        while (f.texels.size() % 4) f.texels.push_back(0);
        hiprz_texture rec{};
        rec.kind = t->kind, rec.width = t->width, rec.height = t->height, rec.offset = uint32_t(f.texels.size());
        rec.scale[0] = t->scale[0], rec.scale[1] = t->scale[1];
        rec.translation[0] = t->translation[0], rec.translation[1] = t->translation[1];
        rec.rotation = t->rotation, rec.cos_rotation = std::cos(t->rotation), rec.sin_rotation = std::sin(t->rotation);
        rec.sampling = t->sampling;
        f.texels.insert(f.texels.end(), t->bitmap.begin(), t->bitmap.end());
        f.textures.push_back(rec);
        f.maps.push_back(t.get());
        return tex_index[t.get()] = int32_t(f.textures.size() - 1);
    };
    std::map<const Material*, int32_t> mat_index;
    auto add_material = [&](const Material& m) {
        hiprz_material r{};
        r.color[0] = m.color.red, r.color[1] = m.color.green, r.color[2] = m.color.blue, r.color[3] = m.color.alpha;
        r.metalness = m.metalness(), r.roughness = m.roughness(), r.emission = m.emission(), r.ior = m.ior(), r.scattering = m.scattering();
        r.texture = tex_id(m.texture), r.normal_map = tex_id(m.normal_map), r.metalness_map = tex_id(m.metalness_map);
        r.roughness_map = tex_id(m.roughness_map), r.emission_map = tex_id(m.emission_map);
        mat_index[&m] = int32_t(f.materials.size());
        f.materials.push_back(r);
    };
    add_material(world.material);
    add_material(world.default_material);
    for (const auto& m : world.materials) add_material(*m);

    // one tree per distinct mesh
    struct MeshTree {
        std::vector<hiprz_node> nodes;
        std::vector<hiprz_tri> tris;
        std::vector<hiprz_tri_attr> attrs;
    };
    std::map<const Mesh*, size_t> mesh_slot;
    std::vector<MeshTree> trees;
    for (const auto& inst : world.instances) {
        if (!inst->mesh || mesh_slot.count(inst->mesh.get())) continue;
        const Mesh& m = *inst->mesh;
        hiprz_mesh_desc d{};
        d.n_vertices = uint32_t(m.vertices.size() / 3), d.vertices = m.vertices.data();
        d.n_texcrds = uint32_t(m.texcrds.size() / 2), d.texcrds = m.texcrds.data();
        d.n_normals = uint32_t(m.normals.size() / 3), d.normals = m.normals.data();
        d.n_triangles = uint32_t(m.tri_materials.size());
        d.tri_vertices = m.tri_vertices.data(), d.tri_texcrds = m.tri_texcrds.data();
        d.tri_normals = m.tri_normals.data(), d.tri_materials = m.tri_materials.data();
        MeshTree t;
        t.nodes.resize(2 * size_t(d.n_triangles) + 1);
        t.tris.resize(d.n_triangles ? d.n_triangles : 1);
        t.attrs.resize(d.n_triangles ? d.n_triangles : 1);
        uint32_t n = 0;
        if (hiprz_build_mesh_tree(&d, t.nodes.data(), uint32_t(t.nodes.size()), &n, t.tris.data(), t.attrs.data()) != HIPRZ_OK)
            throw Exception(HIPRZ_ERR_INVALID, "mesh with out-of-range indices");
        t.nodes.resize(n), t.tris.resize(d.n_triangles), t.attrs.resize(d.n_triangles);
        mesh_slot[&m] = trees.size();
        trees.push_back(std::move(t));
    }

    std::vector<uint8_t> has_mesh;
    for (const auto& inst : world.instances) {
        hiprz_instance r{};
        const Xform own = own_transform(inst->position, inst->rotation, inst->scale), grouped = in_group(*inst);
        store(r, grouped);  // the bounding box always comes from the composed transformation (instance.cpp:125-155)
        r.material_base = uint32_t(f.inst_materials.size());
        uint32_t count = 0;
        for (uint32_t k = 0; k < Instance::materialCapacity(); ++k)
            if (inst->materials[k]) count = k + 1;
        r.material_count = count;
        for (uint32_t k = 0; k < count; ++k) {
            const auto& m = inst->materials[k];
            if (m && !mat_index.count(m.get())) throw Exception(HIPRZ_ERR_INVALID, "instance uses a material that is not in the world");
            f.inst_materials.push_back(m ? mat_index[m.get()] : -1);
        }
        if (inst->mesh) hiprz_instance_bounds(inst->mesh->vertices.data(), uint32_t(inst->mesh->vertices.size() / 3), &r);
        if (world.group_transforms == World::GroupTransforms::Cpu) store(r, own);  // ... but the CPU kernel takes rays into the instance's OWN one (cpu_engine_kernel.cpp:308)
        has_mesh.push_back(inst->mesh ? 1 : 0);
        f.instances.push_back(r);
    }

    const uint32_t n_inst = uint32_t(f.instances.size());
    if (n_inst) {
        f.nodes.resize(2 * size_t(n_inst) + 1);
        f.tlas_order.resize(n_inst);
        uint32_t n = 0, n_order = 0;
        hiprz_build_world_tree(f.instances.data(), has_mesh.data(), n_inst, f.nodes.data(), uint32_t(f.nodes.size()), &n,
                               f.tlas_order.data(), &n_order);
        f.nodes.resize(n), f.tlas_order.resize(n_order);
    }
    std::vector<uint32_t> roots;
    for (auto& t : trees) {
        const uint32_t node_base = uint32_t(f.nodes.size()), tri_base = uint32_t(f.tris.size());
        roots.push_back(node_base);
        for (auto n : t.nodes) {
            n.begin += (n.meta & HIPRZ_NODE_LEAF) ? tri_base : node_base;
            f.nodes.push_back(n);
        }
        f.tris.insert(f.tris.end(), t.tris.begin(), t.tris.end());
        f.tri_attrs.insert(f.tri_attrs.end(), t.attrs.begin(), t.attrs.end());
    }
    for (size_t i = 0; i < world.instances.size(); ++i)
        if (world.instances[i]->mesh) f.instances[i].blas_root = roots[mesh_slot[world.instances[i]->mesh.get()]];

    flatten_lights(world, f);
    return f;
}

namespace {
hiprz_mesh_desc mesh_desc(const Mesh& m) {
    hiprz_mesh_desc d{};
    d.n_vertices = uint32_t(m.vertices.size() / 3), d.vertices = m.vertices.data();
    d.n_texcrds = uint32_t(m.texcrds.size() / 2), d.texcrds = m.texcrds.data();
    d.n_normals = uint32_t(m.normals.size() / 3), d.normals = m.normals.data();
    d.n_triangles = uint32_t(m.tri_materials.size());
    d.tri_vertices = m.tri_vertices.data(), d.tri_texcrds = m.tri_texcrds.data();
    d.tri_normals = m.tri_normals.data(), d.tri_materials = m.tri_materials.data();
    return d;
}
}  // namespace

FlatScene flattenMotion(const World& world, const std::vector<uint32_t>& uploaded_sources) {
    FlatScene f;
    // the meshes in flatten()'s order; every mesh's triangles in the order they were uploaded in
    std::map<const Mesh*, size_t> seen;
    size_t cursor = 0;
    for (const auto& inst : world.instances) {
        if (!inst->mesh || seen.count(inst->mesh.get())) continue;
        seen[inst->mesh.get()] = seen.size();
        const hiprz_mesh_desc d = mesh_desc(*inst->mesh);
        if (cursor + d.n_triangles > uploaded_sources.size()) return FlatScene{};
        const size_t base = f.tris.size();
        f.tris.resize(base + d.n_triangles), f.tri_attrs.resize(base + d.n_triangles);
        if (d.n_triangles &&
            hiprz_fill_triangles(&d, uploaded_sources.data() + cursor, d.n_triangles, f.tris.data() + base, f.tri_attrs.data() + base) != HIPRZ_OK)
            return FlatScene{};
        cursor += d.n_triangles;
    }
    if (cursor != uploaded_sources.size()) return FlatScene{};
    for (const auto& inst : world.instances) {
        hiprz_instance r{};
        const Xform own = own_transform(inst->position, inst->rotation, inst->scale), grouped = in_group(*inst);
        store(r, grouped);
        if (inst->mesh) hiprz_instance_bounds(inst->mesh->vertices.data(), uint32_t(inst->mesh->vertices.size() / 3), &r);
        if (world.group_transforms == World::GroupTransforms::Cpu) store(r, own);
        f.instances.push_back(r);
    }
    return f;
}

FlatScene flattenShading(const World& world) {
    // the map indices must be those of the uploaded scene: textures are numbered in first-use order over world material, default
    // material and the world's materials — exactly what flatten() does, so the numbering is replayed without copying any texels
    FlatScene f;
    std::map<const TextureBuffer*, int32_t> tex_index;
    auto tex_id = [&](const std::shared_ptr<TextureBuffer>& t) -> int32_t {
        if (!t) return -1;
        auto it = tex_index.find(t.get());
        if (it != tex_index.end()) return it->second;
        const int32_t id = int32_t(tex_index.size());
        f.maps.push_back(t.get());
        return tex_index[t.get()] = id;
    };
    auto add_material = [&](const Material& m) {
        hiprz_material r{};
        r.color[0] = m.color.red, r.color[1] = m.color.green, r.color[2] = m.color.blue, r.color[3] = m.color.alpha;
        r.metalness = m.metalness(), r.roughness = m.roughness(), r.emission = m.emission(), r.ior = m.ior(), r.scattering = m.scattering();
        r.texture = tex_id(m.texture), r.normal_map = tex_id(m.normal_map), r.metalness_map = tex_id(m.metalness_map);
        r.roughness_map = tex_id(m.roughness_map), r.emission_map = tex_id(m.emission_map);
        f.materials.push_back(r);
    };
    add_material(world.material);
    add_material(world.default_material);
    for (const auto& m : world.materials) add_material(*m);
    flatten_lights(world, f);
    return f;
}

hiprz_camera cameraRecord(const Camera& cam) {
    const float eps = std::numeric_limits<float>::epsilon();
    hiprz_camera c{};
    put3(c.position, cam.position);
    float rot[3];
    put3(rot, cam.rotation);
    hiprz_axes_look_at(rot, c.x_axis, c.y_axis, c.z_axis);  // camera.cpp:95-100
    c.width = std::max(cam.width, 1u), c.height = std::max(cam.height, 1u);
    c.fov = std::min(std::max(cam.fov, eps), 3.14159265358979f - eps);  // camera.cpp:100-110
    c.tan_half_fov = std::tan(c.fov * 0.5f);
    c.aspect_ratio = float(c.width) / float(c.height);
    c.near_far[0] = std::max(cam.near_plane, eps);
    c.near_far[1] = std::max(cam.far_plane, c.near_far[0] + eps);
    c.focal_distance = std::max(cam.focal_distance, eps);
    c.aperture = std::max(cam.aperture, eps);
    c.exposure_time = std::max(cam.exposure_time, eps);
    return c;
}

// ---- Engine ----
Engine::Engine(int device, int streams) : m_device(device) {
    int rc;
    if (streams > 1) {
        const std::vector<int> ids(size_t(streams), device);
        rc = hiprz_create_multi(&m_ctx, ids.data(), streams);
    } else {
        rc = hiprz_create(&m_ctx, device);
        m_streams_pending = streams == 0;
    }
    if (rc != HIPRZ_OK) throw Exception(rc, std::string("HIPGPU backend unavailable: ") + hiprz_last_error(nullptr));
    check(hiprz_set_tree(m_ctx, m_tree));
}
Engine::Engine(const std::vector<int>& devices) : m_device(devices.empty() ? 0 : devices[0]) {
    const int rc = hiprz_create_multi(&m_ctx, devices.data(), int(devices.size()));
    if (rc != HIPRZ_OK) throw Exception(rc, std::string("HIPGPU backend unavailable: ") + hiprz_last_error(nullptr));
    check(hiprz_set_tree(m_ctx, m_tree));
}
Engine::~Engine() {
    if (m_meter) hiprz_noise_destroy(m_meter);
    if (m_query) hiprz_query_destroy(m_query);
    if (m_order) hiprz_order_destroy(m_order);
    if (m_bake) hiprz_bake_destroy(m_bake);
    if (m_atlas) hiprz_atlas_destroy(m_atlas);
    if (m_light) hiprz_light_destroy(m_light);
    if (m_gather) hiprz_gather_destroy(m_gather);
    if (m_probe) hiprz_probe_destroy(m_probe);
    if (m_smooth) hiprz_smooth_destroy(m_smooth);
    if (m_field) hiprz_field_destroy(m_field);
    if (m_place) hiprz_place_destroy(m_place);
    if (m_view) hiprz_view_destroy(m_view);
    hiprz_destroy(m_ctx);
}

void Engine::check(int rc) {
    if (rc != HIPRZ_OK) throw Exception(rc, hiprz_last_error(m_ctx));
}
void Engine::mode(uint32_t compat_flags) {
    std::lock_guard<std::mutex> lock(m_mutex);
    check(hiprz_set_mode(m_ctx, compat_flags));  // reprojection works over several streams / devices: the context assembles the whole previous frame
    m_mode = compat_flags;
}
void Engine::shardMode(ShardMode mode) {
    std::lock_guard<std::mutex> lock(m_mutex);
    m_streams_pending = false;  // the context stays as it is: the mode is about ITS parts
    check(hiprz_set_shard_mode(m_ctx, uint32_t(mode)));
}
void Engine::setDenoise(const hiprz_denoise_params* params) {
    std::lock_guard<std::mutex> lock(m_mutex);
    // the context's variance estimate is on exactly while the parameters ask for the variance-guided filter or renderUntil measures with it
    // (a change restarts accumulation)
    check(hiprz_set_variance(m_ctx, m_measuring || (params && (params->flags & HIPRZ_DENOISE_VARIANCE)) ? 1 : 0));
    check(hiprz_set_denoise(m_ctx, params));
    m_denoise = params != nullptr;
    if (params) m_denoise_params = *params;
}

void Engine::setMeasuring(bool enabled) {
    std::lock_guard<std::mutex> lock(m_mutex);
    m_measuring = enabled;
    check(hiprz_set_variance(m_ctx, wantVariance()));
}

void Engine::noise(hiprz_noise_summary& out, float threshold, uint32_t min_batches) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (m_camera_records.empty()) throw Exception(HIPRZ_ERR_STATE, "noise: no frame has been rendered");
    check(hiprz_select_camera(m_ctx, 0u));
    const void *accum = nullptr, *variance = nullptr;
    check(hiprz_variance_device(m_ctx, &variance));  // refuses first while the estimate is off
    check(hiprz_accum_device(m_ctx, &accum));
    if (!m_meter)
        if (const int rc = hiprz_noise_create(&m_meter, m_device); rc != HIPRZ_OK) throw Exception(rc, hiprz_noise_last_error(nullptr));
    const hiprz_camera& cam = m_camera_records[0];
    const hiprz_noise_params params{cam.aperture, cam.exposure_time, threshold, min_batches};
    const int rc = hiprz_noise_measure(m_meter, accum, variance, cam.width, cam.height, &params, hiprz_stream(m_ctx), &out, nullptr);
    if (m_camera_records.size() > 1) check(hiprz_select_camera(m_ctx, uint32_t(m_camera_records.size() - 1)));  // where renderWorld left it
    if (rc != HIPRZ_OK) throw Exception(rc, hiprz_noise_last_error(m_meter));
}

hiprz_query* Engine::query() {
    if (!m_query)
        if (const int rc = hiprz_query_create(&m_query, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_query_last_error(nullptr));
    return m_query;
}

hiprz_order* Engine::order() {
    if (!m_order)
        if (const int rc = hiprz_order_create(&m_order, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_order_last_error(nullptr));
    return m_order;
}

std::vector<hiprz_hit> Engine::castRays(const std::vector<hiprz_ray>& rays, bool normalize, bool ordered) {
    std::lock_guard<std::mutex> lock(m_mutex);
    std::vector<hiprz_hit> hits(rays.size());
    if (rays.empty()) return hits;
    const uint32_t flags = normalize ? HIPRZ_QUERY_NORMALIZE : 0u;
    if (ordered) {
        hiprz_order* o = order();
        if (const int rc = hiprz_order_closest_host(o, rays.data(), rays.size(), flags, hits.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_order_last_error(o));
        return hits;
    }
    hiprz_query* q = query();
    const int rc = hiprz_query_closest_host(q, rays.data(), rays.size(), flags, hits.data());
    if (rc != HIPRZ_OK) throw Exception(rc, hiprz_query_last_error(q));
    return hits;
}

std::vector<uint32_t> Engine::occluded(const std::vector<hiprz_ray>& rays, bool normalize, bool ordered) {
    std::lock_guard<std::mutex> lock(m_mutex);
    std::vector<uint32_t> out(rays.size());
    if (rays.empty()) return out;
    const uint32_t flags = normalize ? HIPRZ_QUERY_NORMALIZE : 0u;
    if (ordered) {
        hiprz_order* o = order();
        if (const int rc = hiprz_order_occluded_host(o, rays.data(), rays.size(), flags, out.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_order_last_error(o));
        return out;
    }
    hiprz_query* q = query();
    const int rc = hiprz_query_occluded_host(q, rays.data(), rays.size(), flags, out.data());
    if (rc != HIPRZ_OK) throw Exception(rc, hiprz_query_last_error(q));
    return out;
}

hiprz_bake* Engine::baker(uint32_t K, uint32_t S) {
    if (!m_bake)
        if (const int rc = hiprz_bake_create(&m_bake, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_bake_last_error(nullptr));
    if (K != m_bake_k || S != m_bake_s) {  // the cosine table of (K, S), kept until another is asked for
        std::vector<float> table(4 * size_t(K) * S);
        if (const int rc = hiprz_bake_cosine_directions(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "bakeOcclusion: K is not one of 16 .. 1024 (powers of two) or S is not in 1..64");
        if (const int rc = hiprz_bake_set_directions(m_bake, table.data(), K, S); rc != HIPRZ_OK) throw Exception(rc, hiprz_bake_last_error(m_bake));
        m_bake_k = K, m_bake_s = S;
    }
    return m_bake;
}

std::vector<hiprz_bake_texel> Engine::bakeOcclusion(const std::vector<hiprz_bake_point>& points, uint32_t K, uint32_t S, uint32_t seed) {
    std::lock_guard<std::mutex> lock(m_mutex);
    baker(K, S);
    std::vector<hiprz_bake_texel> out(points.size());
    if (points.empty()) return out;
    if (const int rc = hiprz_bake_occlusion_host(m_bake, points.data(), points.size(), seed, out.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_bake_last_error(m_bake));
    return out;
}

Engine::BakedAtlas Engine::bakeAtlas(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, uint32_t K, uint32_t S, uint32_t seed, uint32_t rings,
                                     float near_, float far_) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (parts.empty()) throw Exception(HIPRZ_ERR_INVALID, "bakeAtlas: an atlas needs at least one part");
    hiprz_bake* b = baker(K, S);
    atlasWith(parts, width, height, near_, far_, "bakeAtlas");
    const auto atlas_check = [this](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_atlas_last_error(m_atlas));
    };
    // the points stay on the device: baked into the handle's own records on the context's stream, dilated there, read once
    const size_t texels = size_t(width) * height;
    void* records = hiprz_atlas_records_device(m_atlas);
    if (const int rc = hiprz_bake_occlusion(b, hiprz_atlas_points_device(m_atlas), texels, seed, static_cast<hiprz_bake_texel*>(records), nullptr); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_bake_last_error(b));
    atlas_check(hiprz_atlas_dilate(m_atlas, records, rings, nullptr, nullptr));
    BakedAtlas out;
    out.width = width, out.height = height;
    out.texels.resize(texels), out.samples.resize(texels), out.ring.resize(texels);
    atlas_check(hiprz_atlas_read_records_host(m_atlas, out.texels.data(), out.ring.data()));
    atlas_check(hiprz_atlas_read_host(m_atlas, nullptr, out.samples.data()));
    return out;
}

hiprz_light* Engine::lighter(uint32_t K, uint32_t S) {
    if (!m_light)
        if (const int rc = hiprz_light_create(&m_light, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_light_last_error(nullptr));
    if (K != m_light_k || S != m_light_s) {  // the disk table of (K, S), kept until another is asked for
        std::vector<float> table(2 * size_t(K) * S);
        if (const int rc = hiprz_light_disk_samples(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "bakeLight: K is not a power of two in 1..1024 or S is not in 1..64");
        if (const int rc = hiprz_light_set_samples(m_light, table.data(), K, S); rc != HIPRZ_OK) throw Exception(rc, hiprz_light_last_error(m_light));
        m_light_k = K, m_light_s = S;
    }
    return m_light;
}

std::vector<hiprz_light_texel> Engine::bakeLight(const std::vector<hiprz_bake_point>& points, uint32_t K, uint32_t S, uint32_t seed, const hiprz_light_range* range) {
    std::lock_guard<std::mutex> lock(m_mutex);
    lighter(K, S);
    std::vector<hiprz_light_texel> out(points.size());
    if (points.empty()) return out;
    if (const int rc = hiprz_light_bake_host(m_light, points.data(), points.size(), seed, range, out.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_light_last_error(m_light));
    return out;
}

hiprz_atlas* Engine::atlasWith(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, float near_, float far_, const char* what) {
    if (!m_atlas)
        if (const int rc = hiprz_atlas_create(&m_atlas, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_atlas_last_error(nullptr));
    const auto atlas_check = [this](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_atlas_last_error(m_atlas));
    };
    atlas_check(hiprz_atlas_begin(m_atlas, width, height));
    size_t base = 0;
    for (const AtlasPart& part : parts) {  // ids numbered through the list
        if (base > 0xFFFFFFFFull) throw Exception(HIPRZ_ERR_INVALID, std::string(what) + ": more than 2^32 triangles");
        atlas_check(hiprz_atlas_add_host(m_atlas, part.charts.data(), part.charts.size(), uint32_t(base), part.instance, near_, far_));
        base += part.charts.size();
    }
    return m_atlas;
}

Engine::LitAtlas Engine::bakeLightAtlas(const std::vector<AtlasPart>& parts, uint32_t width, uint32_t height, uint32_t K, uint32_t S, uint32_t seed, uint32_t rings,
                                        float near_, float far_, const hiprz_light_range* range, const hiprz_smooth_params* smooth) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (parts.empty()) throw Exception(HIPRZ_ERR_INVALID, "bakeLightAtlas: an atlas needs at least one part");
    hiprz_light* l = lighter(K, S);
    atlasWith(parts, width, height, near_, far_, "bakeLightAtlas");
    const auto atlas_check = [this](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_atlas_last_error(m_atlas));
    };
    // the points stay on the device: baked into the handle's own records on the context's stream, dilated there, read once
    const size_t texels = size_t(width) * height;
    void* records = hiprz_atlas_records_device(m_atlas);
    if (const int rc = hiprz_light_bake(l, hiprz_atlas_points_device(m_atlas), texels, seed, range, static_cast<hiprz_light_texel*>(records), nullptr); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_light_last_error(l));
    if (smooth)  // in place, between the bake and the dilation: the gutters take smoothed values
        if (const int rc = hiprz_smooth_texels(smoother(), hiprz_atlas_points_device(m_atlas), records, width, height, smooth, records, nullptr); rc != HIPRZ_OK)
            throw Exception(rc, hiprz_smooth_last_error(m_smooth));
    atlas_check(hiprz_atlas_dilate(m_atlas, records, rings, nullptr, nullptr));
    LitAtlas out;
    out.width = width, out.height = height;
    out.texels.resize(texels), out.samples.resize(texels), out.ring.resize(texels);
    atlas_check(hiprz_atlas_read_records_host(m_atlas, out.texels.data(), out.ring.data()));
    atlas_check(hiprz_atlas_read_host(m_atlas, nullptr, out.samples.data()));
    return out;
}

hiprz_smooth* Engine::smoother() {
    if (!m_smooth)
        if (const int rc = hiprz_smooth_create(&m_smooth, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_smooth_last_error(nullptr));
    return m_smooth;
}

std::vector<Engine::Record> Engine::smoothTexels(const std::vector<hiprz_bake_point>& points, const std::vector<Record>& records, uint32_t width, uint32_t height,
                                                 const hiprz_smooth_params& params) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (points.size() != size_t(width) * height || records.size() != points.size()) throw Exception(HIPRZ_ERR_INVALID, "smoothTexels: points and records are width x height each");
    std::vector<Record> out(records.size());
    if (const int rc = hiprz_smooth_texels_host(smoother(), points.data(), records.data(), width, height, &params, out.data()); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_smooth_last_error(m_smooth));
    return out;
}

Engine::ChartMap Engine::chartMap(const std::vector<AtlasPart>& parts, uint32_t n_instances) {
    ChartMap map;
    map.base.assign(n_instances, HIPRZ_GATHER_NONE);
    for (const AtlasPart& part : parts) {  // ids numbered through the list, as atlasWith numbers them
        if (part.instance >= n_instances) throw Exception(HIPRZ_ERR_INVALID, "chartMap: a part names an instance the world does not have");
        if (map.base[part.instance] != HIPRZ_GATHER_NONE) throw Exception(HIPRZ_ERR_INVALID, "chartMap: an instance is in two parts");
        if (map.uv.size() + part.charts.size() > HIPRZ_GATHER_MAX_CHARTS) throw Exception(HIPRZ_ERR_INVALID, "chartMap: more charts than there are ids");
        map.base[part.instance] = uint32_t(map.uv.size());
        for (const hiprz_atlas_tri& t : part.charts) map.uv.push_back(hiprz_gather_chart{t.u1, t.v1, t.u2, t.v2, t.u3, t.v3, {0.0f, 0.0f}});
    }
    return map;
}

hiprz_gather* Engine::gatherer(uint32_t K, uint32_t S, const ChartMap& charts) {
    if (!m_gather)
        if (const int rc = hiprz_gather_create(&m_gather, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_gather_last_error(nullptr));
    if (K != m_gather_k || S != m_gather_s) {  // the cosine table of (K, S), kept until another is asked for
        std::vector<float> table(4 * size_t(K) * S);
        if (const int rc = hiprz_bake_cosine_directions(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "gather: K is not one of 16 .. 1024 (powers of two) or S is not in 1..64");
        if (const int rc = hiprz_gather_set_directions(m_gather, table.data(), K, S); rc != HIPRZ_OK) throw Exception(rc, hiprz_gather_last_error(m_gather));
        m_gather_k = K, m_gather_s = S;
    }
    if (const int rc = hiprz_gather_set_charts(m_gather, charts.base.data(), uint32_t(charts.base.size()), charts.uv.data(), uint32_t(charts.uv.size())); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_gather_last_error(m_gather));
    return m_gather;
}

std::vector<hiprz_probe_sh> Engine::bakeProbes(const std::vector<hiprz_bake_point>& probes, const std::vector<Record>& source, uint32_t width, uint32_t height,
                                               const ChartMap& charts, uint32_t K, uint32_t S, uint32_t light_K, uint32_t light_S, uint32_t seed, const float* sky,
                                               const hiprz_light_range* range, bool direct) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (source.size() != size_t(width) * height) throw Exception(HIPRZ_ERR_INVALID, "bakeProbes: the source is not width x height records");
    if (!m_probe)
        if (const int rc = hiprz_probe_create(&m_probe, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_probe_last_error(nullptr));
    hiprz_probe* p = m_probe;
    const auto check_probe = [p](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_probe_last_error(p));
    };
    if (K != m_probe_k || S != m_probe_s) {  // the sphere table of (K, S), kept until another is asked for
        std::vector<float> table(4 * size_t(K) * S);
        if (const int rc = hiprz_probe_sphere_directions(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "bakeProbes: K is not one of 16 .. 1024 (powers of two) or S is not in 1..64");
        check_probe(hiprz_probe_set_directions(p, table.data(), K, S));
        m_probe_k = K, m_probe_s = S;
    }
    if (direct && (light_K != m_probe_light_k || light_S != m_probe_light_s)) {
        std::vector<float> disk(2 * size_t(light_K) * light_S);
        if (const int rc = hiprz_light_disk_samples(light_K, light_S, disk.data()); rc != HIPRZ_OK) throw Exception(rc, "bakeProbes: light_K is not a power of two in 1..1024 or light_S is not in 1..64");
        check_probe(hiprz_probe_set_samples(p, disk.data(), light_K, light_S));
        m_probe_light_k = light_K, m_probe_light_s = light_S;
    }
    check_probe(hiprz_probe_set_charts(p, charts.base.data(), uint32_t(charts.base.size()), charts.uv.data(), uint32_t(charts.uv.size())));
    std::vector<hiprz_probe_sh> out(probes.size());
    if (probes.empty()) return out;
    const float black[3] = {0.0f, 0.0f, 0.0f};
    check_probe(hiprz_probe_gather_host(p, probes.data(), probes.size(), seed, source.data(), width, height, sky ? sky : black, out.data()));
    if (direct) check_probe(hiprz_probe_light_host(p, probes.data(), probes.size(), seed, range, out.data(), out.data()));
    return out;
}

std::array<float, 3> Engine::probeIrradiance(const hiprz_probe_sh& sh, const float n[3]) {
    std::array<float, 3> out{};
    hiprz_probe_irradiance(&sh, n, out.data());
    return out;
}

hiprz_field* Engine::fielder() {
    if (!m_field)
        if (const int rc = hiprz_field_create(&m_field, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_field_last_error(nullptr));
    return m_field;
}

std::vector<hiprz_field_vis> Engine::bakeVisibility(const std::vector<hiprz_bake_point>& probes, float reach, uint32_t K, uint32_t S, uint32_t seed) {
    std::lock_guard<std::mutex> lock(m_mutex);
    hiprz_field* f = fielder();
    if (K != m_field_k || S != m_field_s) {  // the sphere table of (K, S), kept until another is asked for
        std::vector<float> table(4 * size_t(K) * S);
        if (const int rc = hiprz_probe_sphere_directions(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "bakeVisibility: K is not one of 64 .. 1024 (powers of two) or S is not in 1..64");
        if (const int rc = hiprz_field_set_directions(f, table.data(), K, S); rc != HIPRZ_OK) throw Exception(rc, hiprz_field_last_error(f));
        m_field_k = K, m_field_s = S;
    }
    std::vector<hiprz_field_vis> out(probes.size());
    if (probes.empty()) return out;
    if (const int rc = hiprz_field_visibility_host(f, probes.data(), probes.size(), seed, reach, out.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_field_last_error(f));
    return out;
}

std::vector<hiprz_bake_point> Engine::placeProbes(const std::vector<hiprz_bake_point>& probes, const hiprz_place_params& params, std::vector<hiprz_place_record>* records, uint32_t K,
                                                  uint32_t S, uint32_t seed) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (!m_place)
        if (const int rc = hiprz_place_create(&m_place, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_place_last_error(nullptr));
    if (K != m_place_k || S != m_place_s) {  // the sphere table of (K, S), kept until another is asked for
        std::vector<float> table(4 * size_t(K) * S);
        if (const int rc = hiprz_probe_sphere_directions(K, S, table.data()); rc != HIPRZ_OK) throw Exception(rc, "placeProbes: K is not one of 64 .. 1024 (powers of two) or S is not in 1..64");
        if (const int rc = hiprz_place_set_directions(m_place, table.data(), K, S); rc != HIPRZ_OK) throw Exception(rc, hiprz_place_last_error(m_place));
        m_place_k = K, m_place_s = S;
    }
    std::vector<hiprz_bake_point> out(probes.size());
    if (records) records->assign(probes.size(), hiprz_place_record{});
    if (probes.empty()) return out;
    if (const int rc = hiprz_place_probes_host(m_place, probes.data(), probes.size(), seed, &params, out.data(), records ? records->data() : nullptr); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_place_last_error(m_place));
    return out;
}

std::vector<hiprz_field_result> Engine::lookupField(const hiprz_field_grid& grid, const std::vector<hiprz_bake_point>& probes, const std::vector<hiprz_probe_sh>& sh,
                                                    const std::vector<hiprz_field_vis>& vis, const std::vector<hiprz_bake_point>& points, const hiprz_field_params& params) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (sh.size() != probes.size() || (!vis.empty() && vis.size() != probes.size())) throw Exception(HIPRZ_ERR_INVALID, "lookupField: one record per probe");
    hiprz_field* f = fielder();
    std::vector<hiprz_field_result> out(points.size());
    if (points.empty()) return out;
    if (const int rc = hiprz_field_lookup_host(f, &grid, probes.data(), sh.data(), vis.empty() ? nullptr : vis.data(), probes.size(), &params, points.data(), points.size(), out.data());
        rc != HIPRZ_OK)
        throw Exception(rc, hiprz_field_last_error(f));
    return out;
}

std::vector<hiprz_view_pixel> Engine::bakedView(const std::vector<Record>& source, uint32_t width, uint32_t height, const ChartMap& charts, const hiprz_view_field* field,
                                                const float* sky, uint32_t filter, std::vector<float>* image) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (source.size() != size_t(width) * height) throw Exception(HIPRZ_ERR_INVALID, "bakedView: the source is not width x height records");
    if (!m_view)
        if (const int rc = hiprz_view_create(&m_view, m_ctx); rc != HIPRZ_OK) throw Exception(rc, hiprz_view_last_error(nullptr));
    if (const int rc = hiprz_view_set_charts(m_view, charts.base.data(), uint32_t(charts.base.size()), charts.uv.data(), uint32_t(charts.uv.size())); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_view_last_error(m_view));
    if (m_camera_records.empty()) throw Exception(HIPRZ_ERR_STATE, "bakedView: no world has been rendered");
    const hiprz_camera& cam = m_camera_records.back();  // the camera renderWorld left selected
    std::vector<hiprz_view_pixel> out(size_t(cam.width) * cam.height);
    if (image) image->assign(4u * out.size(), 0.0f);
    if (out.empty()) return out;
    const float black[3] = {0.0f, 0.0f, 0.0f};
    const hiprz_view_params params{filter, {0u, 0u, 0u}};
    if (const int rc = hiprz_view_pixels_host(m_view, source.data(), width, height, field, sky ? sky : black, &params, out.data(), image ? image->data() : nullptr); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_view_last_error(m_view));
    return out;
}

std::vector<hiprz_gather_texel> Engine::gather(const std::vector<hiprz_bake_point>& points, const std::vector<Record>& source, uint32_t width, uint32_t height,
                                               const ChartMap& charts, uint32_t K, uint32_t S, uint32_t seed, const float* sky) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (source.size() != size_t(width) * height) throw Exception(HIPRZ_ERR_INVALID, "gather: the source is not width x height records");
    hiprz_gather* g = gatherer(K, S, charts);
    std::vector<hiprz_gather_texel> out(points.size());
    if (points.empty()) return out;
    const float black[3] = {0.0f, 0.0f, 0.0f};
    if (const int rc = hiprz_gather_texels_host(g, points.data(), points.size(), seed, source.data(), width, height, sky ? sky : black, out.data()); rc != HIPRZ_OK)
        throw Exception(rc, hiprz_gather_last_error(g));
    return out;
}

Engine::BouncedAtlas Engine::bakeBounceAtlas(const std::vector<AtlasPart>& parts, uint32_t n_instances, uint32_t width, uint32_t height, const std::vector<Record>& albedo,
                                             const std::vector<Record>& emission, uint32_t bounces, uint32_t K, uint32_t S, uint32_t light_K, uint32_t light_S, uint32_t seed,
                                             uint32_t rings, const float* sky, float near_, float far_, const hiprz_smooth_params* smooth) {
    std::lock_guard<std::mutex> lock(m_mutex);
    const size_t texels = size_t(width) * height;
    if (parts.empty()) throw Exception(HIPRZ_ERR_INVALID, "bakeBounceAtlas: an atlas needs at least one part");
    if (bounces < 1u) throw Exception(HIPRZ_ERR_INVALID, "bakeBounceAtlas: a bounce bake takes at least one bounce");
    if (albedo.size() != texels || (!emission.empty() && emission.size() != texels)) throw Exception(HIPRZ_ERR_INVALID, "bakeBounceAtlas: albedo and emission are width x height records");
    hiprz_light* l = lighter(light_K, light_S);
    hiprz_gather* g = gatherer(K, S, chartMap(parts, n_instances));
    atlasWith(parts, width, height, near_, far_, "bakeBounceAtlas");
    const auto atlas_check = [this](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_atlas_last_error(m_atlas));
    };
    const auto gather_check = [g](int rc) {
        if (rc != HIPRZ_OK) throw Exception(rc, hiprz_gather_last_error(g));
    };
    std::vector<hiprz_bake_point> points(texels);
    atlas_check(hiprz_atlas_read_host(m_atlas, points.data(), nullptr));
    BouncedAtlas out;
    out.width = width, out.height = height;
    out.direct.resize(texels), out.indirect.resize(texels), out.ring.resize(texels);
    if (const int rc = hiprz_light_bake_host(l, points.data(), texels, seed, nullptr, out.direct.data()); rc != HIPRZ_OK) throw Exception(rc, hiprz_light_last_error(l));
    // with `smooth`: direct once, right after its bake, and every bounce's indirect right after its gather, in place
    const auto smoothed = [&](void* records) {
        if (!smooth) return;
        if (const int rc = hiprz_smooth_texels_host(smoother(), points.data(), records, width, height, smooth, records); rc != HIPRZ_OK)
            throw Exception(rc, hiprz_smooth_last_error(m_smooth));
    };
    smoothed(out.direct.data());
    const float black[3] = {0.0f, 0.0f, 0.0f};
    std::vector<Record> source(texels);
    for (uint32_t b = 0; b < bounces; ++b) {
        gather_check(hiprz_gather_compose_host(g, out.direct.data(), b ? out.indirect.data() : nullptr, albedo.data(), emission.empty() ? nullptr : emission.data(), source.data(), texels));
        atlas_check(hiprz_atlas_dilate_host(m_atlas, source.data(), rings, nullptr));
        gather_check(hiprz_gather_texels_host(g, points.data(), texels, seed, source.data(), width, height, sky ? sky : black, out.indirect.data()));
        smoothed(out.indirect.data());
    }
    atlas_check(hiprz_atlas_dilate_host(m_atlas, out.direct.data(), rings, nullptr));
    atlas_check(hiprz_atlas_dilate_host(m_atlas, out.indirect.data(), rings, out.ring.data()));
    return out;
}

Engine::NoiseResult Engine::renderUntil(World& world, const RenderConfig& cfg, float target, uint32_t max_passes, uint32_t min_batches) {
    if (max_passes < 1u || min_batches < 2u) throw Exception(HIPRZ_ERR_INVALID, "renderUntil: max_passes must be at least 1 and min_batches at least 2");
    setMeasuring(true);
    NoiseResult r{};
    const uint32_t rpp = std::max(cfg.tracing.rpp, 1u);
    bool measured = false;
    for (uint32_t calls = 1; r.passes < max_passes && !r.met; ++calls) {
        renderWorld(world, cfg, true, true);
        r.passes += rpp, measured = false;
        if (calls >= min_batches) {
            noise(r.summary, 1.0f / 255.0f, min_batches);
            measured = true;
            r.met = r.summary.estimated == r.summary.pixels && r.summary.tile_rms_max <= double(target);
        }
    }
    if (!measured) {  // fewer calls than min_batches: the frame as it stands (it may have been accumulating before this call)
        noise(r.summary, 1.0f / 255.0f, min_batches);
        r.met = r.summary.estimated == r.summary.pixels && r.summary.tile_rms_max <= double(target);
    }
    return r;
}
void Engine::tree(uint32_t tree) {
    std::lock_guard<std::mutex> lock(m_mutex);
    check(hiprz_set_tree(m_ctx, tree));
    m_tree = tree;
    m_last_world = nullptr;  // takes effect at the next scene upload: force one
}

void Engine::deliver(Camera& camera, const World& world, uint32_t sequence) {
    hiprz_frame f{};
    check(hiprz_read_frame(m_ctx, sequence, &f));
    const size_t n = size_t(f.width) * f.height;
    camera.image_buffer.assign(f.rgba8, f.rgba8 + n * 4);
    camera.depth_buffer.assign(f.depth, f.depth + n);
    camera.ray_count = f.ray_count;
    // Kernel::rayCast after every frame (cpu_engine_renderer.cpp:176; cuda_engine_core.cu:164-181): the instance and the instance's
    // material slot the ray through the camera's ray-cast pixel meets at the first-hit depth (hiprz_present cast it on the device)
    const hiprz_raycast hit = f.hit;
    camera.raycasted_instance.reset(), camera.raycasted_material.reset();
    if (hit.instance >= 0 && size_t(hit.instance) < world.instances.size()) {
        camera.raycasted_instance = world.instances[size_t(hit.instance)];
        if (hit.material_slot >= 0 && uint32_t(hit.material_slot) < Instance::materialCapacity())
            camera.raycasted_material = camera.raycasted_instance->materials[size_t(hit.material_slot)];
    }
}

std::vector<Camera*> Engine::enabledCameras(World& world) const {  // cpu_engine_renderer.cpp:97-100: every enabled camera
    std::vector<Camera*> out;
    if (world.camera.enabled) out.push_back(&world.camera);
    for (auto& c : world.cameras)
        if (c && c->enabled) out.push_back(c.get());
    return out;
}

void Engine::renderWorld(World& world, const RenderConfig& cfg, bool /*block*/, bool sync) {
    std::lock_guard<std::mutex> lock(m_mutex);
    if (m_deferred) {  // error of the previous, already returned, asynchronous frame
        Exception e = *m_deferred;
        m_deferred.reset();
        throw e;
    }
    if (m_streams_pending) {  // the first world: as many streams on the GPU as suit it
        m_streams_pending = false;
        const int streams = defaultStreams(world);
        if (streams > 1) {
            hiprz_ctx* several = nullptr;
            const std::vector<int> ids(size_t(streams), m_device);
            if (hiprz_create_multi(&several, ids.data(), streams) == HIPRZ_OK) {
                if (m_query) hiprz_query_destroy(m_query);  // bound to the context that goes
                m_query = nullptr;
                if (m_order) hiprz_order_destroy(m_order);
                m_order = nullptr;
                if (m_bake) hiprz_bake_destroy(m_bake);
                m_bake = nullptr, m_bake_k = m_bake_s = 0;
                if (m_atlas) hiprz_atlas_destroy(m_atlas);
                m_atlas = nullptr;
                if (m_light) hiprz_light_destroy(m_light);
                m_light = nullptr, m_light_k = m_light_s = 0;
                if (m_gather) hiprz_gather_destroy(m_gather);
                m_gather = nullptr, m_gather_k = m_gather_s = 0;
                if (m_probe) hiprz_probe_destroy(m_probe);
                m_probe = nullptr, m_probe_k = m_probe_s = m_probe_light_k = m_probe_light_s = 0;
                if (m_smooth) hiprz_smooth_destroy(m_smooth);
                m_smooth = nullptr;
                if (m_field) hiprz_field_destroy(m_field);
                m_field = nullptr, m_field_k = m_field_s = 0;
                if (m_place) hiprz_place_destroy(m_place);
                m_place = nullptr, m_place_k = m_place_s = 0;
                if (m_view) hiprz_view_destroy(m_view);
                m_view = nullptr;
                hiprz_destroy(m_ctx);
                m_ctx = several;
                check(hiprz_set_mode(m_ctx, m_mode));
                check(hiprz_set_tree(m_ctx, m_tree));
                check(hiprz_set_variance(m_ctx, wantVariance()));
                check(hiprz_set_denoise(m_ctx, m_denoise ? &m_denoise_params : nullptr));
            }
        }
    }
    const std::vector<Camera*> cameras = enabledCameras(world);
    // pipelined frames of the previous non-sync call: every camera still enabled gets its frame once this call's renders are enqueued
    // (the first call after a (re)start has none, and leaves the buffers as they are)
    std::vector<PendingFrame> pending;
    pending.swap(m_pending_frames);
    if (!m_pending_readback) pending.clear();
    m_pending_readback = false;
    pending.erase(std::remove_if(pending.begin(), pending.end(),
                                 [&](const PendingFrame& p) {
                                     return std::find(cameras.begin(), cameras.end(), p.camera) == cameras.end() ||
                                            p.slot >= m_camera_slots.size() || m_camera_slots[p.slot] != p.camera;
                                 }),
                  pending.end());
    auto deliver_pending = [&](size_t slot) {  // before what would free a camera's frame slots: hand out its frame now
        for (auto it = pending.begin(); it != pending.end();)
            if (slot == SIZE_MAX || it->slot == slot) {
                check(hiprz_select_camera(m_ctx, uint32_t(it->slot)));
                deliver(*it->camera, world, it->sequence);
                it = pending.erase(it);
            } else {
                ++it;
            }
    };
    // re-mirror what changed; any change restarts accumulation (cpu_engine_renderer.cpp:108-112)
    bool moved_in_place = false;
    if (world.isMoved() && !world.isModified() && m_last_world == &world && world.instances.size() == m_uploaded_instances) {
        // an animation frame: where the device built the trees it refits them and rebuilds the world tree; no tree is built on the host
        uint32_t tree = HIPRZ_TREE_REFERENCE;
        if (hiprz_tree(m_ctx, &tree) == HIPRZ_OK && (tree == HIPRZ_TREE_DEVICE || tree == HIPRZ_TREE_DEVICE_SAH)) {
            const FlatScene motion = flattenMotion(world, m_uploaded_sources);
            if (motion.instances.size() == m_uploaded_instances && motion.tris.size() == m_uploaded_sources.size()) {
                if (!motion.tris.empty()) check(hiprz_update_triangles(m_ctx, 0u, uint32_t(motion.tris.size()), motion.tris.data(), motion.tri_attrs.data()));
                if (!motion.instances.empty()) check(hiprz_update_instances(m_ctx, motion.instances.data(), uint32_t(motion.instances.size())));
                // a refitted tree keeps the topology it was built with: every kRebuildEvery-th moved frame the device builds the trees again
                // over the vertices it holds (config D twisted by three radians per unit: 28 ms per step refitted, 12 ms rebuilt)
                if (++m_moved_frames % kRebuildEvery == 0u) check(hiprz_rebuild_trees(m_ctx, tree));
                moved_in_place = true;
            }
        }
    }
    if (world.isMoved() && !moved_in_place) world.makeModified();  // no device trees (or another topology): an ordinary modification
    world.makeUnmoved();
    if (world.isModified() || m_last_world != &world) {
        const FlatScene flat = flatten(world);
        const hiprz_scene view = flat.view();
        check(hiprz_upload_scene(m_ctx, &view));
        world.makeUnmodified(), world.makeShadingUnmodified();
        m_last_world = &world;
        m_uploaded_maps = flat.maps;
        m_uploaded_sources.resize(flat.tris.size());
        for (size_t k = 0; k < flat.tris.size(); ++k) m_uploaded_sources[k] = flat.tris[k].source_index;
        m_uploaded_instances = flat.instances.size();
        m_moved_frames = 0;
    } else if (world.isShadingModified()) {  // materials / lights only: replaced in place, no tree is touched
        const FlatScene shading = flattenShading(world);
        // flattenShading numbers the maps in first-use order; those indices mean something only if they name the SAME map objects in
        // the same order as the uploaded scene's (a material re-pointed at another uploaded map changes the first-use order, a new
        // map has no texels on the device at all): otherwise the whole scene goes up again, as the adapter does (WorldAdapter::refresh)
        if (shading.maps == m_uploaded_maps) {
            check(hiprz_update_shading(m_ctx, shading.materials.data(), uint32_t(shading.materials.size()), shading.spot_lights.data(),
                                       uint32_t(shading.spot_lights.size()), shading.direct_lights.data(), uint32_t(shading.direct_lights.size())));
        } else {
            const FlatScene flat = flatten(world);
            const hiprz_scene view = flat.view();
            check(hiprz_upload_scene(m_ctx, &view));
            m_uploaded_maps = flat.maps;
            m_uploaded_sources.resize(flat.tris.size());
            for (size_t k = 0; k < flat.tris.size(); ++k) m_uploaded_sources[k] = flat.tris[k].source_index;
            m_uploaded_instances = flat.instances.size();
        }
        world.makeShadingUnmodified();
    }
    hiprz_config c{};
    c.max_depth = cfg.tracing.max_depth, c.rpp = cfg.tracing.rpp;
    c.spot_samples = std::max<uint32_t>(cfg.light_sampling.spot_light, 1u);      // cuda_kernel_data.cu:23-31
    c.direct_samples = std::max<uint32_t>(cfg.light_sampling.direct_light, 1u);
    c.seed = cfg.seed;
    check(hiprz_set_config(m_ctx, &c));
    // one frame state per enabled camera, in the order the reference iterates them
    bool slots_changed = m_camera_slots.size() != cameras.size();
    for (size_t k = 0; !slots_changed && k < cameras.size(); ++k) slots_changed = m_camera_slots[k] != cameras[k];
    if (slots_changed) {
        deliver_pending(SIZE_MAX);
        const size_t n_slots = std::max<size_t>(cameras.size(), 1);
        check(hiprz_set_camera_count(m_ctx, uint32_t(n_slots)));
        m_presented.resize(n_slots, 0u), m_frame_sizes.resize(n_slots, {0u, 0u});
        m_camera_slots.assign(cameras.begin(), cameras.end());
        m_camera_records.assign(cameras.size(), hiprz_camera{});
        for (Camera* cam : cameras) cam->makeModified();
    }
    for (size_t k = 0; k < cameras.size(); ++k) {
        Camera& cam = *cameras[k];
        check(hiprz_select_camera(m_ctx, uint32_t(k)));
        if (cam.isModified()) {
            const hiprz_camera rec = cameraRecord(cam);
            // an upload restarts accumulation (cpu_engine_renderer.cpp:108-112); a camera that only moved its ray-cast pixel
            // (Camera::rayCastPixel: MakeModified, not RequestUpdate) keeps accumulating in both reference engines
            if (slots_changed || std::memcmp(&rec, &m_camera_records[k], sizeof rec) != 0) {
                if (m_frame_sizes[k] != std::make_pair(rec.width, rec.height)) {  // new frame slots, the sequence restarts
                    deliver_pending(k);
                    m_presented[k] = 0u, m_frame_sizes[k] = {rec.width, rec.height};
                }
                check(hiprz_upload_camera(m_ctx, &rec));
                m_camera_records[k] = rec;
            }
            check(hiprz_set_temporal_blend(m_ctx, cam.temporal_blend));
            cam.makeUnmodified();
        }
        check(hiprz_render(m_ctx, std::max(cfg.tracing.rpp, 1u)));
        // tone map, assemble and ray-cast the frame on the device, copy it to pinned memory on the context's copy stream: enqueued only
        check(hiprz_present(m_ctx, cam.ray_cast_pixel[0], cam.ray_cast_pixel[1]));
        const uint32_t sequence = ++m_presented[k];
        if (sync) deliver(cam, world, sequence);
        else m_pending_frames.push_back({k, &cam, sequence});
    }
    // not sync: nothing of this call's frames has been waited for — the buffers are filled by the next call, and a device fault would
    // surface at that call's first hip* return.  The previous call's frames travelled to the host while these renders were enqueued.
    if (!sync) {
        for (const PendingFrame& p : pending) {
            check(hiprz_select_camera(m_ctx, uint32_t(p.slot)));
            deliver(*p.camera, world, p.sequence);
        }
        if (!pending.empty() && !cameras.empty()) check(hiprz_select_camera(m_ctx, uint32_t(cameras.size() - 1)));
        m_pending_readback = true;
    }
}

std::string Engine::timingsString() {
    std::lock_guard<std::mutex> lock(m_mutex);
    char buf[4096];
    if (hiprz_timings(m_ctx, buf, sizeof buf) != HIPRZ_OK) return {};
    return buf;
}

}  // namespace RayZath::Hip
