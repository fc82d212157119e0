// hiprz_scene_host.hpp — the pure-host half of scene mirroring: validation, the derived walk tables, and the ONE place where the device
// layout of a record is written down (interleaved boxes, the packed instance record, the hot blob's sections, the shadow rays' tree).
// Standard library, include/hiprz.h and hiprz_end.hpp only, no HIP header: hiprz_scene_host.cpp compiles with a plain host compiler, and
// tests/test_scene_pack.py runs it without a GPU under a sanitizer.  hiprz_scene.hip copies what this unit packs and binds DScene to it;
// hiprz_device.hpp reads the same layouts on the device.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "hiprz.h"
#include "hiprz_end.hpp"

namespace hiprz {

constexpr uint32_t kLeafMax = 4u;  // device-built mesh trees: one quad entry of the cooperative triangle phase (hiprz_build.hip)
constexpr uint32_t kPairRecordBytes = RZ_PAIR_RECORD_BYTES;  // two triangles of a single-leaf mesh, interleaved (PackedScene::pair_section)
constexpr uint16_t kPairNone = 0xFFFFu;                       // table entry of an instance whose mesh has no pair record
constexpr size_t kPairSectionLimit = 8u * 0xFFFEu;            // what a 16-bit table entry in units of 8 bytes can address

// one mesh of a scene whose trees are built on the device (hiprz_build.hip)
struct DeviceMesh {
    uint32_t tri_first = 0, n_tris = 0;  // its triangles in the device order
    uint32_t ref_first = 0;              // ... and in the uploaded snapshot's order (a mesh's triangles are contiguous in both)
    uint32_t region = 0xFFFFFFFFu;       // slot of its root in the node arrays (RZ_END: too small to build, stays one leaf)
    uint32_t leaf_slot = 0xFFFFFFFFu;    // ... the slot of that one leaf (the uploaded placeholder), whose box a refit fits again
    uint32_t n_slots = 0;                // nodes emitted
    float bb_min[3] = {0, 0, 0}, bb_max[3] = {0, 0, 0};
};
// Capacity of the node arrays of a scene whose mesh trees are built on the device: the uploaded prefix + per mesh a region of 2n - 1
// slots starting at an odd index (its child pairs then start at even indices: one 128-byte line per pair of 64-byte walk records).
uint32_t device_build_regions(std::vector<DeviceMesh>& meshes, uint32_t first_free_slot);

// ---- record layouts ----
// shared-reciprocal division is exact only for coordinates that are 0 or in [2^-60, 2^40)
inline bool coord_ok(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    const uint32_t e = (b >> 23) & 0xFFu;
    return (b & 0x7FFFFFFFu) == 0u || (e >= 127u - 60u && e < 127u + 40u);
}
// device copies keep every box interleaved, (min.x, max.x, min.y, max.y, min.z, max.z), so one axis' two plane distances are one
// packed operand of the box test (hiprz_device.hpp: box_hit).  A node's bb_min[3] and bb_max[3] are contiguous.
inline void interleave_box(hiprz_node& n) {
    const float v[6] = {n.bb_min[0], n.bb_max[0], n.bb_min[1], n.bb_max[1], n.bb_min[2], n.bb_max[2]};
    std::memcpy(n.bb_min, v, 12), std::memcpy(n.bb_max, v + 3, 12);
}
inline void deinterleave_box(hiprz_node& n) {
    const float v[6] = {n.bb_min[0], n.bb_min[1], n.bb_min[2], n.bb_max[0], n.bb_max[1], n.bb_max[2]};
    n.bb_min[0] = v[0], n.bb_max[0] = v[1], n.bb_min[1] = v[2], n.bb_max[1] = v[3], n.bb_min[2] = v[4], n.bb_max[2] = v[5];
}
// The packed instance record: the placement of `in` (position, scale, axes, world box) written into `d` the way the walks read it — pad0
// flags a unit scale (x / 1.0f == x: the walk skips the division), the box is interleaved like a node's with max.y parked in pad2.
// Everything else of `d` (blas_root, the material table) stays.
inline void pack_instance_placement(hiprz_instance& d, const hiprz_instance& in) {
    const float v[6] = {in.bb_min[0], in.bb_max[0], in.bb_min[1], in.bb_max[1], in.bb_min[2], in.bb_max[2]};
    const uint32_t unit = (in.scale[0] == 1.0f && in.scale[1] == 1.0f && in.scale[2] == 1.0f) ? 1u : 0u;
    std::memcpy(d.position, in.position, 12), std::memcpy(d.scale, in.scale, 12);
    std::memcpy(d.x_axis, in.x_axis, 12), std::memcpy(d.y_axis, in.y_axis, 12), std::memcpy(d.z_axis, in.z_axis, 12);
    d.pad0 = unit;
    d.bb_min[0] = v[0], d.bb_min[1] = v[1], d.bb_min[2] = v[2];
    std::memcpy(&d.pad2, &v[3], 4);
    d.bb_max[0] = v[4], d.bb_max[1] = v[5], d.bb_max[2] = 0.0f;
}
struct InstanceBox {
    float mn[3], mx[3];
};
inline InstanceBox packed_instance_box(const hiprz_instance& d) {  // ... and its box read back
    float max_y;
    std::memcpy(&max_y, &d.pad2, 4);
    return InstanceBox{{d.bb_min[0], d.bb_min[2], d.bb_max[0]}, {d.bb_min[1], max_y, d.bb_max[1]}};
}
// a material's maps index `textures` (or are unset) and have the kind their slot reads
bool material_maps_ok(const hiprz_material& m, const hiprz_texture* textures, uint32_t n_textures);

// ---- validation and the derived walk tables ----
// Everything the kernels will dereference is checked here, on the host, before any launch: a
// bad index or a cyclic tree would otherwise fault or hang the GPU.  Also derives the skip links,
// the world-tree leaves and the tree depths the upload needs.
struct SceneCheck {
    std::string error;
    std::vector<uint8_t> reachable;  // nodes some walk can get to (a snapshot may hold others: they are never followed)
    std::vector<uint32_t> skip;
    std::vector<uint32_t> world_leaves;
    uint32_t world_depth = 0, mesh_depth = 0;
};
int check_scene(const hiprz_scene* sc, SceneCheck& out);

// Device-side tables derived from a validated scene (pure host): relayouted nodes + links (reference order and per octant).
struct DerivedTables {
    std::vector<uint32_t> new_index;
    std::vector<hiprz_node> dnodes;
    std::vector<uint32_t> dskip;
    std::vector<uint32_t> dskip8;  // [node][octant]: skip links of the front-to-back mesh walk (hiprz_device.hpp: fetch_node_ordered)
};
int derive_tables(const hiprz_scene* sc, SceneCheck& chk, DerivedTables& out);

// ---- upload, stage by stage ----
// Which trees the upload walks (hiprz_set_tree).  HIPRZ_TREE_REFERENCE keeps the caller's snapshot; any other mode rewrites it — new
// nodes, triangles and their attributes in the new leaf order, every triangle remembering its position in the reference's order — into
// the vectors below, and `scene` points at them.  `chk` holds the check of the snapshot on entry and of `scene` on return.
struct ChosenTrees {
    hiprz_scene scene{};
    uint32_t tree = HIPRZ_TREE_REFERENCE;  // of `scene`: a mode that could not be applied under HIPRZ_TREE_AUTO fell back to the reference's
    bool own_trees = false;                // `scene` is the rewritten snapshot
    bool identity_order = false;           // ... whose triangles kept the snapshot's order (they were not copied)
    std::vector<hiprz_node> nodes;
    std::vector<hiprz_tri> tris;
    std::vector<hiprz_tri_attr> attrs;
    std::vector<hiprz_instance> instances;
    ChosenTrees() = default;
    ChosenTrees(const ChosenTrees&) = delete;  // `scene` points into the vectors of THIS object
    ChosenTrees& operator=(const ChosenTrees&) = delete;
    bool device_trees() const { return own_trees && tree == HIPRZ_TREE_DEVICE; }
};
// `lds_limit`: under HIPRZ_TREE_AUTO a scene whose records fit this many bytes keeps the snapshot's trees.  HIPRZ_ERR_INVALID + `error`.
int choose_trees(const hiprz_scene* sc, uint32_t tree_mode, size_t lds_limit, SceneCheck& chk, ChosenTrees& out, std::string& error);

// What the device is going to hold, as plain host values: no DScene, no device pointer.
struct PackedScene {
    // hot blob: one buffer, 16-B aligned sections in this order; hot_bytes = blob.size()
    std::vector<uint8_t> blob;
    uint32_t off_nodes = 0, off_tlas_order = 0, off_instances = 0, off_tris = 0, off_tri_attrs = 0, off_materials = 0, off_inst_materials = 0;
    std::vector<uint32_t> new_index;          // snapshot node -> device node
    std::vector<hiprz_node> nodes;            // relayouted, boxes interleaved
    std::vector<uint32_t> skip;               // reference-order skip links (node_capacity entries)
    std::vector<uint32_t> nodes64;            // front-to-back walk: 64-B records, node + the 8 octant links (node_capacity records)
    std::vector<hiprz_instance> instances;    // packed (pack_instance_placement), blas_root remapped
    std::vector<uint32_t> world_members;      // the instances of the world tree, by rising id
    bool fast_div = true;                     // every box coordinate is coord_ok
    float bounds_min[3] = {0, 0, 0}, bounds_scale[3] = {0, 0, 0};  // the world root's box, 32 cells per axis
    uint32_t tlas_root = 0;
    bool flat_world = false;                  // the world tree is one leaf of at most 8 instances
    // Pair records: what the one-leaf walk's triangle loop reads (hiprz_device.hpp: binned_visit).  NOT part of
    // `blob`: the upload places the section directly behind the blob in the device's hot buffer, and DScene::hot_bytes is the total,
    // so whatever stages or sizes the hot buffer carries the section along.  Empty unless the world is flat, the snapshot's own trees
    // are walked and some instance's mesh is ONE leaf.  Layout: a table of ((n_instances + 3) & ~3) 16-bit words — instance id -> where
    // its mesh's first pair record starts, in units of 8 bytes from the section's start, kPairNone for a mesh that is not one leaf
    // (instances of one mesh share records) —, then per such mesh ceil(n / 2) records of kPairRecordBytes, 8-byte aligned: nine float2
    // {a, b} = v1.x, v1.y, v1.z, edge1.x .. edge2.z of triangles begin + 2p (a) and begin + 2p + 1 (b) of the leaf, bit copies of the
    // blob's triangle records; the last record of an odd leaf repeats a in b.  Zeros pad the section to a multiple of 16 bytes.
    // Why as small as this (no padding to 80-byte records, no 32-bit table): config B's five workgroups per CU have 592 bytes of LDS to
    // spare below 25 allocation blocks of 1 280 bytes each — its eight records and eight table entries are 592 bytes; at 672 bytes the
    // fifth workgroup no longer fits and the kernel loses 5 %.
    // The section cannot go stale: only scenes with the snapshot's trees are ever staged in LDS (hiprz_plan.cpp: use_lds_scene), and
    // hiprz_update_triangles / hiprz_rebuild_trees require HIPRZ_TREE_DEVICE — the triangles of a scene that has a section change
    // through hiprz_upload_scene alone, which packs again.
    std::vector<uint8_t> pair_section;
    size_t hot_bytes() const { return blob.size() + pair_section.size(); }  // what the device's hot buffer holds
    // device-built trees (ChosenTrees::device_trees): room behind the uploaded prefix for the world tree (2 * instances + 1 slots) and
    // for every mesh tree (2 * triangles - 1 slots); regions start at odd slots, their child pairs at even ones
    std::vector<DeviceMesh> device_meshes;
    std::vector<uint32_t> instance_mesh;      // instance -> index into device_meshes (RZ_END: no mesh)
    uint32_t world_region = 0, node_capacity = 0;
};
// From a validated snapshot (`trees.scene` passed check_scene, `derived` are its tables, consumed).  HIPRZ_ERR_INVALID + `error`.
// `pair_records` = false leaves pair_section empty and everything else what it is with it (tests/test_pair_records.py compares the two).
int pack_scene(const ChosenTrees& trees, DerivedTables&& derived, PackedScene& out, std::string& error, bool pair_records = true);

// Surface records: what analyze_intersection (hiprz_device.hpp) derives from (instance, triangle, side hit) alone, computed once per
// upload for the kernels that stage the scene in LDS (RZ_SURFACE_RECORDS).  NOT part of `blob` and NOT counted in hot_bytes(): the upload
// places the section 16-byte aligned behind the hot buffer's hot_bytes(), nothing stages it (every LDS figure of the launch plan stays
// what it is; one more byte of LDS costs config B its fifth workgroup per CU) and the kernels read it from global memory through
// DScene::hot.  Layout: a table of ((n_instances + 3) & ~3) 32-bit words — instance id -> (index of its first record pair - first
// triangle of its mesh), so the pair of a hit is table[instance] + hit.triangle —, then per (instance of the world tree, triangle of its mesh) two records
// of kSurfaceRecordBytes, the side hit from inside (external = 0) first: normal.xyz, bits(surface_material), mapped_normal.xyz,
// bits(flags).  behind_material follows from the side (external ? surface_material : HIPRZ_MATERIAL_WORLD).  A mesh's triangles are the
// range [lowest, highest) its tree's leaves cover.
// Every record is computed by analyze_intersection's literal sequence for ITS side — the slot clamp and the HIPRZ_MATERIAL_DEFAULT rule;
// normalized(transform_forward((face_normal * ef) / scale)); normalized(transform_forward(face_normal / scale)) * ef — because the two
// sides are not each other's negation: (+0) + (-0) is +0 under either sign, so an axis-aligned wall's zeros differ in sign between the
// sides, and the sign reaches 1 / d of the next segment's slab tests.  Host and device agree bit for bit (-ffp-contract=off, no fast
// math, correctly rounded division and square root on both) for finite, normal numbers only: kSurfaceNormalValid and
// kSurfaceMappedValid are both clear when an input or an intermediate is subnormal, infinite or NaN (a zero-area triangle among them),
// kSurfaceMappedValid also for a triangle with HIPRZ_TRI_HAS_NORMALS (its mapped normal is interpolated per hit); a lane that finds a
// flag clear computes that normal as before.
// Built for every scene that may be staged: the snapshot's own trees and hot_bytes() + stack_entries * 1 KiB <= lds_limit (the widest
// rule of hiprz_plan.cpp: use_lds_scene); empty otherwise.  Such a scene's geometry and instances change through hiprz_upload_scene
// alone (see pair_section), and hiprz_update_shading changes no material id, so the section cannot go stale.
constexpr uint32_t kSurfaceRecordBytes = RZ_SURFACE_RECORD_BYTES;
constexpr uint32_t kSurfaceNormalValid = RZ_SURFACE_NORMAL_VALID, kSurfaceMappedValid = RZ_SURFACE_MAPPED_VALID;
std::vector<uint8_t> pack_surface_section(const ChosenTrees& trees, const PackedScene& packed, uint32_t stack_entries, size_t lds_limit);

// Instances enter their mesh at the root the device built (where it built one); returns the nodes the builds emitted.
uint32_t enter_device_roots(std::vector<hiprz_instance>& instances, const std::vector<uint32_t>& instance_mesh, const std::vector<DeviceMesh>& meshes,
                            uint32_t world_slots);

// The shadow rays' own world tree over `members` of the packed `instances`: 2 n 64-byte walk records (root in record 0) and the
// instance ids its leaves index.
void build_shadow_tree(const std::vector<hiprz_instance>& instances, const std::vector<uint32_t>& members, std::vector<uint32_t>& records,
                       std::vector<uint32_t>& order);

}  // namespace hiprz
