// hiprz_scene.hip — scene mirroring of the C-ABI declared in include/hiprz.h: validation, upload, the in-place changes (shading, triangles,
// trees, instances) and the download of the trees.  Everything that needs no device — the checks, the walk tables, the device layout of
// every record — is in hiprz_scene_host.cpp; this unit copies what that one packs, binds DScene to the copies and runs the device
// builders (hiprz_build.hip).  It defines no kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiprz.h"
#include "hiprz_ctx.hpp"
#include "hiprz_device.hpp"
#include "hiprz_scene_host.hpp"

using namespace hiprz;

// Scene calls: a peer on ANOTHER device mirrors the scene itself; a peer on the head's own device (a second stream on the same GPU)
// walks the head's copy — one scene blob per device, however many streams share it.
#define RZ_FANOUT_OTHER_DEVICES(c, call)                                                                                       \
    for (hiprz_ctx* p : (c)->peers) {                                                                                         \
        if (p->device == (c)->device) continue;                                                                               \
        const int rz_rc = (call);                                                                                             \
        if (rz_rc != HIPRZ_OK) return fail(c, rz_rc, "device " + std::to_string(p->device) + ": " + p->error);              \
    }

namespace {

// a same-device peer takes over the head's view of the scene (pointers into the head's buffers, every derived figure)
void adopt_scene(hiprz_ctx* p, const hiprz_ctx* head) {
    p->dscene = head->dscene, p->have_scene = head->have_scene, p->stack_entries = head->stack_entries, p->lds_scene = head->lds_scene;
    p->n_nodes = head->n_nodes, p->flat_world = head->flat_world, p->n_textures = head->n_textures, p->scene_tree = head->scene_tree;
    p->tree_mode = head->tree_mode, p->device_sah = head->device_sah, p->build_sah = head->build_sah, p->n_tris = head->n_tris, p->n_tlas_order = head->n_tlas_order;
    p->scene_shared = true;
    invalidate_graphs(p);
    p->reset_pending = true;
    for (auto& f : p->parked) f.reset_pending = true;
}
void share_scene_with_streams(hiprz_ctx* c) {
    for (hiprz_ctx* p : c->peers)
        if (p->device == c->device) adopt_scene(p, c);
}

// Every call that changes the scene of a context holds one of these.  On entry the streams on the head's own device, which walk the
// head's copy, have finished reading what the call is about to replace (the hazard PartStaging guards for frame buffers); whatever way
// the call ends, they see what the head holds then.  What else a call does is its own and named where the guard is made: only the
// upload invalidates the head's graphs up front and re-resolves the sharing streams' pipeline on exit.
struct SceneChange {
    enum : unsigned { kInPlace = 0u, kInvalidateGraphs = 1u, kResolvePeerPipelines = 2u };
    hiprz_ctx* c;
    unsigned effects;
    SceneChange(hiprz_ctx* ctx, unsigned effects_) : c(ctx), effects(effects_) {
        for (hiprz_ctx* p : c->peers)
            if (p->device == c->device) (void)hipStreamSynchronize(p->stream);
        if (effects & kInvalidateGraphs) invalidate_graphs(c);
    }
    ~SceneChange() {
        share_scene_with_streams(c);
        if (effects & kResolvePeerPipelines)
            for (hiprz_ctx* p : c->peers)
                if (p->device == c->device) resolve_pipeline(p);
    }
    SceneChange(const SceneChange&) = delete;
    SceneChange& operator=(const SceneChange&) = delete;
};

// A change of the scene failed half way, in place or in an upload past the point of no return (a device-built tree the host refused to prove terminating, a device error): the node
// tables, the triangle order or the instance roots may be part old, part new — there is no scene any more.  hiprz_render then returns
// HIPRZ_ERR_STATE instead of walking tables nobody proved, and the streams that share this device's copy learn the same (SceneChange's destructor).
int scene_lost(hiprz_ctx* c, int rc) {
    c->have_scene = false;
    c->device_meshes.clear(), c->instance_mesh.clear();
    invalidate_graphs(c);
    return rc;
}
int restart_after_geometry_change(hiprz_ctx* c) {
    c->reset_pending = true;  // the world changed: accumulation restarts (cpu_engine_renderer.cpp:108-112), for every camera
    stale_guides(c);
    for (auto& f : c->parked) f.reset_pending = true;
    return HIPRZ_OK;
}
// the host proves every device-built tree before a walk follows it, unless told not to
bool validate_device_trees() { return !std::getenv("HIPRZ_TRUST_DEVICE_TREES"); }
uint32_t env_u32(const char* name, uint32_t otherwise) {
    const char* v = std::getenv(name);
    return v ? uint32_t(std::atoi(v)) : otherwise;
}
// ray reordering key: where only the closest-hit walk follows the sorted order, the origin's cell interleaved with where the ray is
// going groups best (config C, the 6-D Morton code of cell and direction: trace kernel 583 -> 503 us; round 4: the direction on the
// octahedron, E 2 682 -> 2 556 us, C 324 -> 316; then the cell where the ray leaves the world box instead of a direction, E -> 2 400,
// C -> 299); where the deferred shadow rays follow that order too (HIPRZ_SHADOW_SORT=0) they fan out from the origin cell, so the
// origin leads (config E: 86.5 ms per step against 92.6)
uint32_t sort_variant_for(const hiprz_ctx* c, uint32_t n_lights) { return n_lights && c->shadow_sort == 0 ? 0u : 4u; }

// The device half of the shadow rays' own world tree (hiprz_scene_host.cpp: build_shadow_tree), at every upload and every
// hiprz_update_instances.  Buffers are sized once per scene (2 n records), so the DScene a captured graph holds stays valid across updates.
int build_shadow_world_tree(hiprz_ctx* c, const std::vector<hiprz_instance>& dinst, DScene& d) {
    d.shadow_nodes64 = nullptr, d.shadow_order = nullptr, d.shadow_root = RZ_END;
    const std::vector<uint32_t>& members = c->world_members;
    // Where it pays (the living room's pass, wave-level walk on this tree / on the reference's / cooperative walk, ms): 40 instances at 4K 4.20 / 4.34 /
    // 4.75, 100 at 4K 5.91 / 6.13 / 6.65, 100 at 1080p 2.09 / 2.17 / 2.28, 300 at 4K 9.00 / 8.84 / 9.29 — a deep binary tree is a long chain of
    // dependent steps for a wave that crosses many instances; beyond 160 the walk keeps the reference's tree (and the host is spared the build).
    if (!c->shadow_tree || members.empty() || members.size() > 160u) return HIPRZ_OK;
    std::vector<uint32_t> rec, order;
    build_shadow_tree(dinst, members, rec, order);
    (void)hipSetDevice(c->device);
    RZ_HIP(c, c->shadow_nodes64.resize(rec.size()));
    RZ_HIP(c, c->shadow_order.resize(order.size()));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_HIP(c, hipMemcpy(c->shadow_nodes64.ptr, rec.data(), rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    RZ_HIP(c, hipMemcpy(c->shadow_order.ptr, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    d.shadow_nodes64 = reinterpret_cast<const float4*>(c->shadow_nodes64.ptr), d.shadow_order = c->shadow_order.ptr, d.shadow_root = 0u;
    return HIPRZ_OK;
}

// ---- hiprz_upload_scene, stage by stage ----

// every copy of the upload, on the context's stream; synchronous on return (host staging and the caller's arrays may go away)
int copy_scene(hiprz_ctx* c, const hiprz_scene& sc, const PackedScene& packed, const std::vector<uint8_t>& surface_section, bool device_trees) {
    (void)hipSetDevice(c->device);
    if (packed.pair_section.empty() && surface_section.empty()) {
        RZ_HIP(c, c->hot.assign(packed.blob.data(), packed.blob.size(), c->stream));
    } else {
        // the pair records stand directly behind the blob: one hot buffer, staged as a whole (DScene::hot_bytes is the total); the surface
        // records follow 16-byte aligned behind hot_bytes, in the buffer but outside what is counted and staged (hiprz_device.hpp: surface_section)
        std::vector<uint8_t> hot(packed.blob);
        hot.insert(hot.end(), packed.pair_section.begin(), packed.pair_section.end());
        hot.resize((hot.size() + 15u) & ~size_t(15), 0);
        hot.insert(hot.end(), surface_section.begin(), surface_section.end());
        RZ_HIP(c, c->hot.assign(hot.data(), hot.size(), c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));  // (`hot` goes away)
    }
    RZ_HIP(c, c->node_skip.assign(packed.skip.data(), packed.skip.size(), c->stream));
    if (device_trees) {  // the node records of the whole scene in a buffer of their own: the uploaded prefix + room for what the device builds
        hiprz_node unused{};
        unused.meta = HIPRZ_NODE_LEAF;  // slots no build fills stay empty leaves nothing links to
        std::vector<hiprz_node> all(packed.node_capacity, unused);
        std::copy(packed.nodes.begin(), packed.nodes.end(), all.begin());
        RZ_HIP(c, c->dev_nodes.assign(reinterpret_cast<const uint8_t*>(all.data()), all.size() * sizeof(hiprz_node), c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));
    }
    RZ_HIP(c, c->nodes64.assign(packed.nodes64.data(), packed.nodes64.size(), c->stream));
    RZ_HIP(c, c->textures.assign(sc.textures, sc.n_textures, c->stream));
    RZ_HIP(c, c->texels.assign(sc.texels, sc.texel_bytes, c->stream));
    RZ_HIP(c, c->spot_lights.assign(sc.spot_lights, sc.n_spot_lights, c->stream));
    RZ_HIP(c, c->direct_lights.assign(sc.direct_lights, sc.n_direct_lights, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

// the walks' tunables: measured defaults, each with an environment variable for experiments
void bind_tunables(hiprz_ctx* c, DScene& d, uint32_t n_lights) {
    // mesh walk rounds of at most 4 node steps and 8 triangles per lane (measured: D 3 163 -> 2 891 us, C 935 -> 892 us)
    d.walk_k = env_u32("HIPRZ_WALK_K", 4u), d.walk_l = env_u32("HIPRZ_WALK_L", 8u);
    d.walk_h = env_u32("HIPRZ_WALK_H", 65u);  // never: ending the node phase early for a full triangle step measured no gain (D 1 010 vs 999 us)
    d.sort_variant = env_u32("HIPRZ_SORT_KEY", sort_variant_for(c, n_lights));
    // the shadow rays' key: the pixel's set of sample slots (+ 0x100: the shadow kernel's loop over the slots is wave-uniform, a slot few of a
    // wave's pixels hold costs the wave a whole walk; E 40.33 -> 39.85 ms), then the light the ray goes to and the origin's cell in a 64^3
    // grid (+ 0x400; E 38.5 -> 37.8 ms against layout 0 — cell, then direction —, which was the best of the layouts: the rays fan out from the cell)
    d.shadow_variant = env_u32("HIPRZ_SHADOW_KEY", 0x500u);
    // The world and instance levels of the cooperative walks ("while-while" one and two levels above the mesh walk; the order in which a
    // lane meets its instances stays the reference's).  World level: a lane steps through up to 1 + 8 nodes of the world tree per round
    // until it HOLDS a leaf with instances, so that the expensive part — the ray into an instance's space, the mesh walk — runs for many
    // lanes at once instead of for the few that happened to reach a leaf in this step (E, 46 instances: trace kernel 3 010 -> 2 678 us,
    // shade + shadow 2 711 -> 2 636; 1 / 2 / 4 / 8 / 64 further steps: 2 992 / 2 892 / 2 798 / 2 712 / 2 716 us).  Instance level: a lane
    // that misses an instance's box tests the next one in the same round (D 836 -> 803 us; with 4 and more D's lanes reach the big mesh
    // in different rounds, each as long as its longest walk: 1 045 us and worse).  profiles/r03/ab_instance_advance.txt, ab_world_advance.txt
    d.walk_advance = env_u32("HIPRZ_WALK_ADVANCE", 1u);
    d.world_advance = env_u32("HIPRZ_WORLD_ADVANCE", 8u);
}

// DScene and the context's derived figures over the buffers copy_scene filled
void bind_scene(hiprz_ctx* c, const ChosenTrees& trees, const PackedScene& packed, const SceneCheck& chk) {
    const hiprz_scene& sc = trees.scene;
    DScene& d = c->dscene;
    c->stack_entries = chk.world_depth + chk.mesh_depth + 2u;
    d.world_stack_entries = chk.world_depth + 1u;
    d.mesh_stack_entries = chk.mesh_depth + 1u;
    d.off_nodes = packed.off_nodes, d.off_tlas_order = packed.off_tlas_order, d.off_instances = packed.off_instances, d.off_tris = packed.off_tris;
    d.off_tri_attrs = packed.off_tri_attrs, d.off_materials = packed.off_materials, d.off_inst_materials = packed.off_inst_materials;
    d.off_pairs = uint32_t(packed.blob.size());
    d.hot_bytes = uint32_t(packed.hot_bytes());
    d.hot = reinterpret_cast<const float4*>(c->hot.ptr);
    d.nodes = reinterpret_cast<const float4*>(trees.device_trees() ? c->dev_nodes.ptr : c->hot.ptr + d.off_nodes);
    d.tlas_order = reinterpret_cast<const uint32_t*>(c->hot.ptr + d.off_tlas_order);
    d.instances = reinterpret_cast<const float4*>(c->hot.ptr + d.off_instances);
    d.tris = reinterpret_cast<const float4*>(c->hot.ptr + d.off_tris);
    d.tri_attrs = reinterpret_cast<const float4*>(c->hot.ptr + d.off_tri_attrs);
    d.materials = reinterpret_cast<const float4*>(c->hot.ptr + d.off_materials);
    d.inst_materials = reinterpret_cast<const int32_t*>(c->hot.ptr + d.off_inst_materials);
    d.fast_div = packed.fast_div ? 1u : 0u;
    d.textures = reinterpret_cast<const float4*>(c->textures.ptr);
    d.texels = c->texels.ptr;
    d.spot_lights = reinterpret_cast<const float4*>(c->spot_lights.ptr);
    d.direct_lights = reinterpret_cast<const float4*>(c->direct_lights.ptr);
    d.n_instances = sc.n_instances;
    d.tlas_root = packed.tlas_root;
    d.node_skip = c->node_skip.ptr;
    std::memcpy(d.bounds_min, packed.bounds_min, 12), std::memcpy(d.bounds_scale, packed.bounds_scale, 12);
    d.top_count = std::min<uint32_t>(uint32_t(packed.nodes.size()), kTopCacheNodes);
    d.nodes64 = reinterpret_cast<const float4*>(c->nodes64.ptr);
    d.n_spot_lights = sc.n_spot_lights;
    d.n_direct_lights = sc.n_direct_lights;
    bind_tunables(c, d, sc.n_spot_lights + sc.n_direct_lights);
    c->n_nodes = sc.n_nodes;
    c->flat_world = packed.flat_world;
    c->n_textures = sc.n_textures;
    // Stage the blob in LDS when three workgroups per CU (the kernel's register-limited residency)
    // still fit into the CU's 160 KiB together with their traversal stacks.
    c->lds_scene = size_t(d.hot_bytes) + size_t(c->stack_entries) * 1024u + BinnedLds::kFixedBytes <= kLdsSceneLimit;
    c->scene_tree = trees.tree;
    if (trees.own_trees) c->lds_scene = false;  // rebuilt trees are walked front to back on skip links only (ties by reference position)
    c->n_tris = sc.n_tris, c->n_tlas_order = sc.n_tlas_order;
    c->device_meshes.clear(), c->instance_mesh.clear();
    c->world_members = packed.world_members;
}

// HIPRZ_TREE_DEVICE: the world tree and every mesh tree, built by the device into the regions pack_scene planned
int build_device_trees(hiprz_ctx* c, PackedScene& packed) {
    const bool validate = validate_device_trees();
    const uint32_t n_instances = uint32_t(packed.instances.size());
    c->node_capacity = packed.node_capacity, c->world_region = packed.world_region;
    c->device_instances = packed.instances;
    std::vector<uint8_t> has_mesh(n_instances ? n_instances : 1u, 0);
    for (uint32_t i = 0; i < n_instances; ++i) has_mesh[i] = packed.instance_mesh[i] != RZ_END ? 1 : 0;
    RZ_HIP(c, c->has_mesh.assign(has_mesh.data(), has_mesh.size(), c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_HIP(c, c->slot_parent.resize(packed.node_capacity));
    RZ_HIP(c, hipMemsetAsync(c->slot_parent.ptr, 0xFF, size_t(packed.node_capacity) * sizeof(uint32_t), c->stream));  // RZ_END: the single leaves of small meshes have no parent
    if (c->n_tlas_order) {
        const int rc = device_build_world_tree(c, validate);
        if (rc != HIPRZ_OK) return rc;
        c->dscene.tlas_root = packed.world_region;
    }
    const int rc = device_build_mesh_trees(c, packed.device_meshes, packed.instance_mesh, validate);
    if (rc != HIPRZ_OK) return rc;
    c->instance_mesh = packed.instance_mesh;
    c->n_nodes = enter_device_roots(c->device_instances, c->instance_mesh, c->device_meshes, c->world_slots);
    return HIPRZ_OK;
}

}  // namespace

extern "C" {

int hiprz_validate_scene(const hiprz_scene* scene, char* message, size_t len) {
    SceneCheck chk;
    int rc = check_scene(scene, chk);
    if (rc == HIPRZ_OK) {  // also prove that the tables the kernels will follow can be derived and terminate
        DerivedTables derived;
        rc = derive_tables(scene, chk, derived);
    }
    if (message && len) std::snprintf(message, len, "%s", chk.error.c_str());
    return rc;
}

int hiprz_upload_scene(hiprz_ctx* c, const hiprz_scene* sc) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT_OTHER_DEVICES(c, hiprz_upload_scene(p, sc));
    SceneChange change(c, SceneChange::kInvalidateGraphs | SceneChange::kResolvePeerPipelines);
    StageTimer timer;
    std::string error;
    // choose trees: validated, then the snapshot's own or (hiprz_set_tree) a rewritten snapshot, validated again
    SceneCheck chk;
    if (check_scene(sc, chk) != HIPRZ_OK) return fail(c, HIPRZ_ERR_INVALID, "upload_scene: " + chk.error);
    c->build_sah = c->device_sah || c->tree_mode == HIPRZ_TREE_AUTO;
    ChosenTrees trees;
    if (choose_trees(sc, c->tree_mode, kLdsSceneLimit, chk, trees, error) != HIPRZ_OK) return fail(c, HIPRZ_ERR_INVALID, error);
    if (trees.own_trees) c->timings.set("rebuild mesh trees", timer.ms());
    DerivedTables derived;
    if (derive_tables(&trees.scene, chk, derived) != HIPRZ_OK) return fail(c, HIPRZ_ERR_INVALID, "upload_scene: " + chk.error);
    // from here on the device buffers of the previous scene are being replaced: until the new one is complete there is no scene
    // (a failed upload must not leave the old scene's kernels arguments pointing at reallocated buffers)
    c->have_scene = false;
    PackedScene packed;
    if (pack_scene(trees, std::move(derived), packed, error) != HIPRZ_OK) return scene_lost(c, fail(c, HIPRZ_ERR_INVALID, error));
    // what analyze_intersection would derive per hit, for the kernels that stage the scene in LDS (any scene use_lds_scene may ever stage)
    const std::vector<uint8_t> surface_section = pack_surface_section(trees, packed, chk.world_depth + chk.mesh_depth + 2u, kLdsPerCu);
    int rc = copy_scene(c, trees.scene, packed, surface_section, trees.device_trees());
    if (rc != HIPRZ_OK) return scene_lost(c, rc);
    bind_scene(c, trees, packed, chk);
    if (trees.device_trees()) rc = build_device_trees(c, packed);
    if (rc != HIPRZ_OK) return scene_lost(c, rc);
    rc = build_shadow_world_tree(c, packed.instances, c->dscene);  // over the instances of the world tree (those with a mesh)
    if (rc != HIPRZ_OK) return scene_lost(c, rc);
    c->have_scene = true;
    resolve_pipeline(c);
    c->timings.set("upload scene", timer.ms());
    return restart_after_geometry_change(c);
}

// Materials and lights of the uploaded scene changed, geometry did not (the reference's dirty flags per container, updatable.cpp:23-51;
// Cuda::World re-mirrors only modified containers, cuda_world.cu:28-57): the records are replaced in place — no tree is rebuilt,
// re-derived or re-validated.  The material count must be that of the uploaded scene (instances refer to materials by index).
int hiprz_update_shading(hiprz_ctx* c, const hiprz_material* materials, uint32_t n_materials, const hiprz_spot_light* spot_lights,
                         uint32_t n_spot_lights, const hiprz_direct_light* direct_lights, uint32_t n_direct_lights) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT_OTHER_DEVICES(c, hiprz_update_shading(p, materials, n_materials, spot_lights, n_spot_lights, direct_lights, n_direct_lights));
    SceneChange change(c, SceneChange::kInPlace);
    if (!c->have_scene) return fail(c, HIPRZ_ERR_STATE, "update_shading before upload_scene");
    const uint32_t uploaded = (c->dscene.off_inst_materials - c->dscene.off_materials) / uint32_t(sizeof(hiprz_material));
    if (!materials || n_materials < 2u || ((n_materials * sizeof(hiprz_material) + 15u) & ~size_t(15)) != size_t(c->dscene.off_inst_materials - c->dscene.off_materials))
        return fail(c, HIPRZ_ERR_INVALID, "update_shading: the scene was uploaded with " + std::to_string(uploaded) + " material slots");
    if ((n_spot_lights && !spot_lights) || (n_direct_lights && !direct_lights)) return fail(c, HIPRZ_ERR_INVALID, "update_shading: null array with non-zero count");
    std::vector<hiprz_texture> tex(c->n_textures);
    (void)hipSetDevice(c->device);
    if (c->n_textures) RZ_HIP(c, hipMemcpy(tex.data(), c->textures.ptr, sizeof(hiprz_texture) * c->n_textures, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_materials; ++i)
        if (!material_maps_ok(materials[i], tex.data(), c->n_textures))
            return fail(c, HIPRZ_ERR_INVALID, "update_shading: material " + std::to_string(i) + ": map index/kind invalid");
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_HIP(c, hipMemcpy(c->hot.ptr + c->dscene.off_materials, materials, sizeof(hiprz_material) * n_materials, hipMemcpyHostToDevice));
    RZ_HIP(c, c->spot_lights.assign(spot_lights, n_spot_lights, c->stream));
    RZ_HIP(c, c->direct_lights.assign(direct_lights, n_direct_lights, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    c->dscene.spot_lights = reinterpret_cast<const float4*>(c->spot_lights.ptr);
    c->dscene.direct_lights = reinterpret_cast<const float4*>(c->direct_lights.ptr);
    c->dscene.n_spot_lights = n_spot_lights, c->dscene.n_direct_lights = n_direct_lights;
    if (!std::getenv("HIPRZ_SORT_KEY")) c->dscene.sort_variant = sort_variant_for(c, n_spot_lights + n_direct_lights);
    invalidate_graphs(c);
    return restart_after_geometry_change(c);
}

// ---- geometry changes without a host-side tree build (scenes uploaded under HIPRZ_TREE_DEVICE; hiprz_build.hip) ----
int hiprz_update_triangles(hiprz_ctx* c, uint32_t first, uint32_t n, const hiprz_tri* tris, const hiprz_tri_attr* attrs) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT_OTHER_DEVICES(c, hiprz_update_triangles(p, first, n, tris, attrs));
    SceneChange change(c, SceneChange::kInPlace);
    if (!c->have_scene || c->scene_tree != HIPRZ_TREE_DEVICE) return fail(c, HIPRZ_ERR_STATE, "update_triangles: the scene was not uploaded under HIPRZ_TREE_DEVICE");
    if (n == 0u) return HIPRZ_OK;
    if (!tris || !attrs || uint64_t(first) + n > c->n_tris) return fail(c, HIPRZ_ERR_INVALID, "update_triangles: range outside the uploaded triangles");
    for (uint32_t k = 0; k < n; ++k)  // the walks divide by nothing here, but the shading indexes material slots
        if ((tris[k].material_flags & HIPRZ_TRI_MATERIAL_MASK) > 0xFFFFFFu) return fail(c, HIPRZ_ERR_INVALID, "update_triangles: bad material id");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    const int rc = device_update_triangles(c, first, n, tris, attrs);
    if (rc != HIPRZ_OK) return scene_lost(c, rc);
    return restart_after_geometry_change(c);
}

int hiprz_rebuild_trees(hiprz_ctx* c, uint32_t tree) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT_OTHER_DEVICES(c, hiprz_rebuild_trees(p, tree));
    SceneChange change(c, SceneChange::kInPlace);
    if (!c->have_scene || c->scene_tree != HIPRZ_TREE_DEVICE) return fail(c, HIPRZ_ERR_STATE, "rebuild_trees: the scene's trees were not built on the device");
    if (tree != HIPRZ_TREE_DEVICE && tree != HIPRZ_TREE_DEVICE_SAH) return fail(c, HIPRZ_ERR_INVALID, "rebuild_trees: HIPRZ_TREE_DEVICE or HIPRZ_TREE_DEVICE_SAH");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    invalidate_graphs(c);
    c->build_sah = tree == HIPRZ_TREE_DEVICE_SAH;
    // the meshes' bounds as they are now: the box of every root (exact after a refit)
    std::vector<DeviceMesh> meshes = c->device_meshes;
    for (DeviceMesh& m : meshes) {
        const uint32_t root = m.region != RZ_END ? m.region : m.leaf_slot;
        if (root == RZ_END || m.n_tris == 0u) continue;
        hiprz_node rec;
        RZ_HIP(c, hipMemcpy(&rec, c->dev_nodes.ptr + size_t(root) * sizeof(hiprz_node), sizeof rec, hipMemcpyDeviceToHost));
        deinterleave_box(rec);
        std::memcpy(m.bb_min, rec.bb_min, 12), std::memcpy(m.bb_max, rec.bb_max, 12);
    }
    const std::vector<uint32_t> instance_mesh = c->instance_mesh;
    const int rc = device_build_mesh_trees(c, meshes, instance_mesh, validate_device_trees());
    if (rc != HIPRZ_OK) return scene_lost(c, rc);  // nodes, links and the triangle order were being rewritten in place
    c->n_nodes = enter_device_roots(c->device_instances, c->instance_mesh, c->device_meshes, c->world_slots);
    resolve_pipeline(c);
    return restart_after_geometry_change(c);
}

int hiprz_update_instances(hiprz_ctx* c, const hiprz_instance* instances, uint32_t n) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT_OTHER_DEVICES(c, hiprz_update_instances(p, instances, n));
    SceneChange change(c, SceneChange::kInPlace);
    if (!c->have_scene || c->scene_tree != HIPRZ_TREE_DEVICE) return fail(c, HIPRZ_ERR_STATE, "update_instances: the scene was not uploaded under HIPRZ_TREE_DEVICE");
    if (!instances || n != c->dscene.n_instances || n != c->device_instances.size()) return fail(c, HIPRZ_ERR_INVALID, "update_instances: the scene was uploaded with " + std::to_string(c->dscene.n_instances) + " instances");
    bool fast_div = c->dscene.fast_div != 0u;
    for (uint32_t i = 0; i < n; ++i) {
        pack_instance_placement(c->device_instances[i], instances[i]);  // keeps blas_root (the device-built root) and the material table
        for (int a = 0; a < 3; ++a) fast_div = fast_div && coord_ok(instances[i].bb_min[a]) && coord_ok(instances[i].bb_max[a]);
    }
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_HIP(c, hipMemcpy(c->hot.ptr + c->dscene.off_instances, c->device_instances.data(), sizeof(hiprz_instance) * n, hipMemcpyHostToDevice));
    if (!fast_div && c->dscene.fast_div) c->dscene.fast_div = 0u, invalidate_graphs(c);
    if (c->n_tlas_order) {
        const int rc = device_build_world_tree(c, validate_device_trees());
        if (rc != HIPRZ_OK) return scene_lost(c, rc);  // the new instance records and a world tree nobody proved are on the device
    }
    const int rc = build_shadow_world_tree(c, c->device_instances, c->dscene);  // the instances moved: the shadow rays' tree over them again
    if (rc != HIPRZ_OK) return scene_lost(c, rc);
    return restart_after_geometry_change(c);
}

int hiprz_download_trees(hiprz_ctx* c, hiprz_node* nodes_out, uint32_t max_nodes, uint32_t* n_nodes_out, uint32_t* tlas_root_out, uint32_t* tlas_order_out,
                         uint32_t* blas_roots_out, uint32_t* tri_refpos_out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_scene) return fail(c, HIPRZ_ERR_STATE, "download_trees before upload_scene");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    const bool device_trees = c->scene_tree == HIPRZ_TREE_DEVICE;
    const uint32_t n_nodes = device_trees ? c->node_capacity : uint32_t((c->dscene.off_tlas_order - c->dscene.off_nodes) / sizeof(hiprz_node));
    if (n_nodes_out) *n_nodes_out = n_nodes;
    if (tlas_root_out) *tlas_root_out = c->dscene.tlas_root;
    if (nodes_out) {
        if (max_nodes < n_nodes) return fail(c, HIPRZ_ERR_INVALID, "download_trees: " + std::to_string(n_nodes) + " nodes");
        RZ_HIP(c, hipMemcpy(nodes_out, c->dscene.nodes, sizeof(hiprz_node) * n_nodes, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < n_nodes; ++k) deinterleave_box(nodes_out[k]);
    }
    if (tlas_order_out && c->n_tlas_order) RZ_HIP(c, hipMemcpy(tlas_order_out, c->hot.ptr + c->dscene.off_tlas_order, 4u * c->n_tlas_order, hipMemcpyDeviceToHost));
    if (blas_roots_out && c->dscene.n_instances) {
        std::vector<hiprz_instance> inst(c->dscene.n_instances);
        RZ_HIP(c, hipMemcpy(inst.data(), c->hot.ptr + c->dscene.off_instances, sizeof(hiprz_instance) * inst.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < inst.size(); ++i) blas_roots_out[i] = inst[i].blas_root;
    }
    if (tri_refpos_out && c->n_tris) {
        std::vector<hiprz_tri> tris(c->n_tris);
        RZ_HIP(c, hipMemcpy(tris.data(), c->hot.ptr + c->dscene.off_tris, sizeof(hiprz_tri) * tris.size(), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < tris.size(); ++t) tri_refpos_out[t] = tris[t].pad0;
    }
    return HIPRZ_OK;
}

}  // extern "C"
