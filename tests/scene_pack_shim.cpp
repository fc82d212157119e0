// The pure-host half of scene mirroring (rayzath_amd/csrc/hiprz_scene_host.cpp) behind a C interface for tests/test_scene_pack.py: one
// upload's host stages — check, choose trees, derive, pack, shadow tree — and views of everything they produced.
#include <cstdio>
#include <string>
#include <vector>

#include "hiprz_scene_host.hpp"

using namespace hiprz;

namespace {
struct Packed {
    SceneCheck chk;
    ChosenTrees trees;
    PackedScene packed;
    std::vector<float> boxes;  // per instance: the box the accessor reads back from the packed record, (min xyz, max xyz)
    std::vector<uint32_t> shadow_records, shadow_order;
};
}  // namespace

extern "C" {

struct rzp_view {
    const uint8_t* blob;
    uint64_t blob_bytes;
    uint32_t off[7];  // nodes, tlas_order, instances, tris, tri_attrs, materials, inst_materials
    uint32_t tree, own_trees, identity_order, fast_div, tlas_root, node_capacity, world_region, n_device_meshes;
    const hiprz_scene* scene;  // the snapshot that was packed: the caller's, or the rewritten one
    const uint8_t* reachable;
    const uint32_t* new_index;
    const hiprz_node* nodes;
    uint32_t n_nodes;  // relayouted nodes (the scene's + the padding slot)
    const uint32_t* skip;
    const uint32_t* nodes64;
    const hiprz_instance* instances;
    const float* boxes;
    const uint32_t* members;
    uint32_t n_members;
    const uint32_t* shadow_records;
    uint32_t n_shadow_records;
    const uint32_t* shadow_order;
    const DeviceMesh* device_meshes;  // 48-byte records: tri_first, n_tris, ref_first, region, leaf_slot, n_slots, bb_min, bb_max
    const uint32_t* instance_mesh;
};

// lds_limit: what hiprz_upload_scene passes for HIPRZ_TREE_AUTO.  Returns a handle, or null with the refusal in `message`.
void* rzp_pack(const hiprz_scene* sc, uint32_t tree_mode, uint64_t lds_limit, rzp_view* view, char* message, size_t len) {
    auto* p = new Packed();
    std::string error;
    int rc = check_scene(sc, p->chk);
    if (rc != HIPRZ_OK) error = p->chk.error;
    if (rc == HIPRZ_OK) rc = choose_trees(sc, tree_mode, size_t(lds_limit), p->chk, p->trees, error);
    DerivedTables derived;
    if (rc == HIPRZ_OK && (rc = derive_tables(&p->trees.scene, p->chk, derived)) != HIPRZ_OK) error = p->chk.error;
    if (rc == HIPRZ_OK) rc = pack_scene(p->trees, std::move(derived), p->packed, error);
    if (rc != HIPRZ_OK) {
        if (message && len) std::snprintf(message, len, "%s", error.c_str());
        delete p;
        return nullptr;
    }
    const PackedScene& k = p->packed;
    for (const hiprz_instance& in : k.instances) {
        const InstanceBox b = packed_instance_box(in);
        p->boxes.insert(p->boxes.end(), b.mn, b.mn + 3);
        p->boxes.insert(p->boxes.end(), b.mx, b.mx + 3);
    }
    if (!k.world_members.empty()) build_shadow_tree(k.instances, k.world_members, p->shadow_records, p->shadow_order);
    rzp_view v{};
    v.blob = k.blob.data(), v.blob_bytes = k.blob.size();
    const uint32_t off[7] = {k.off_nodes, k.off_tlas_order, k.off_instances, k.off_tris, k.off_tri_attrs, k.off_materials, k.off_inst_materials};
    for (int i = 0; i < 7; ++i) v.off[i] = off[i];
    v.tree = p->trees.tree, v.own_trees = p->trees.own_trees, v.identity_order = p->trees.identity_order, v.fast_div = k.fast_div;
    v.tlas_root = k.tlas_root, v.node_capacity = k.node_capacity, v.world_region = k.world_region, v.n_device_meshes = uint32_t(k.device_meshes.size());
    v.scene = &p->trees.scene, v.reachable = p->chk.reachable.data(), v.new_index = k.new_index.data();
    v.nodes = k.nodes.data(), v.n_nodes = uint32_t(k.nodes.size()), v.skip = k.skip.data(), v.nodes64 = k.nodes64.data();
    v.instances = k.instances.data(), v.boxes = p->boxes.data(), v.members = k.world_members.data(), v.n_members = uint32_t(k.world_members.size());
    v.shadow_records = p->shadow_records.data(), v.n_shadow_records = uint32_t(p->shadow_records.size() / 16u), v.shadow_order = p->shadow_order.data();
    v.device_meshes = k.device_meshes.data(), v.instance_mesh = k.instance_mesh.data();
    *view = v;
    return p;
}

// the box layout, both ways, in place
void rzp_interleave(hiprz_node* nodes, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) interleave_box(nodes[i]);
}
void rzp_deinterleave(hiprz_node* nodes, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) deinterleave_box(nodes[i]);
}
// enter_device_roots as after a device build that emitted n_slots[m] nodes for mesh m: the instances' roots, and the return value
uint32_t rzp_enter_device_roots(void* handle, const uint32_t* n_slots, uint32_t world_slots, uint32_t* blas_roots_out) {
    const PackedScene& k = static_cast<Packed*>(handle)->packed;
    std::vector<DeviceMesh> meshes = k.device_meshes;
    for (size_t m = 0; m < meshes.size(); ++m) meshes[m].n_slots = n_slots[m];
    std::vector<hiprz_instance> instances = k.instances;
    const uint32_t emitted = enter_device_roots(instances, k.instance_mesh, meshes, world_slots);
    for (size_t i = 0; i < instances.size(); ++i) blas_roots_out[i] = instances[i].blas_root;
    return emitted;
}

void rzp_free(void* handle) { delete static_cast<Packed*>(handle); }

}  // extern "C"
