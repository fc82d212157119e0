// The pair section of the packer (rayzath_amd/csrc/hiprz_scene_host.cpp: PackedScene::pair_section) checked on the host alone: scenes
// built here go through every host stage of an upload, and the section that comes out is compared with the blob's triangle records.
// tests/test_pair_records.py compiles this file with hiprz_scene_host.cpp and hiprz_host.cpp under AddressSanitizer and UBSan and runs it
// as a child process.  Prints one line per scene, "pair records: N scenes ok" at the end; any failed check ends it with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiprz_scene_host.hpp"

using namespace hiprz;

namespace {

#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            std::exit(1);                                    \
        }                                                    \
    } while (0)

uint32_t mix(uint32_t v) {
    v ^= v >> 16, v *= 0x7FEB352Du, v ^= v >> 15, v *= 0x846CA68Bu, v ^= v >> 16;
    return v;
}
float coordinate(uint32_t k) { return float(mix(k) >> 8) * (8.0f / 16777216.0f) - 4.0f; }  // 24 random bits in [-4, 4)

struct MeshSpec {
    std::vector<uint32_t> leaves;  // one entry: the root is a leaf of that many triangles; two: an inner root over two leaves
};

// One world: `meshes`, instance i of mesh instance_mesh[i]; the world tree is one leaf of all instances, or (split_world) an inner root
// over two leaves.
struct World {
    std::vector<hiprz_node> nodes;
    std::vector<uint32_t> tlas_order;
    std::vector<hiprz_tri> tris;
    std::vector<hiprz_tri_attr> attrs;
    std::vector<hiprz_instance> instances;
    std::vector<int32_t> inst_materials;
    std::vector<hiprz_material> materials;
    std::vector<uint32_t> mesh_root, mesh_first_tri;
    hiprz_scene scene{};
};

hiprz_node leaf(uint32_t begin, uint32_t count) {
    hiprz_node n{};
    for (int a = 0; a < 3; ++a) n.bb_min[a] = -4.0f, n.bb_max[a] = 4.0f;
    n.begin = begin, n.meta = HIPRZ_NODE_LEAF | count;
    return n;
}
hiprz_node inner(uint32_t first_child) {
    hiprz_node n = leaf(first_child, 0u);
    n.meta = 2u << HIPRZ_NODE_PTYPE_SHIFT;
    return n;
}

void build(World& w, const std::vector<MeshSpec>& meshes, const std::vector<uint32_t>& instance_mesh, bool split_world, uint32_t seed) {
    const uint32_t n_inst = uint32_t(instance_mesh.size());
    if (split_world) {
        w.nodes.push_back(inner(1u));
        w.nodes.push_back(leaf(0u, n_inst / 2u));
        w.nodes.push_back(leaf(n_inst / 2u, n_inst - n_inst / 2u));
    } else {
        w.nodes.push_back(leaf(0u, n_inst));
    }
    for (const MeshSpec& m : meshes) {
        w.mesh_root.push_back(uint32_t(w.nodes.size()));
        w.mesh_first_tri.push_back(uint32_t(w.tris.size()));
        uint32_t total = 0;
        for (uint32_t c : m.leaves) total += c;
        if (m.leaves.size() == 1u) {
            w.nodes.push_back(leaf(uint32_t(w.tris.size()), total));
        } else {
            const uint32_t at = uint32_t(w.nodes.size());
            w.nodes.push_back(inner(at + 1u));
            w.nodes.push_back(leaf(uint32_t(w.tris.size()), m.leaves[0]));
            w.nodes.push_back(leaf(uint32_t(w.tris.size()) + m.leaves[0], m.leaves[1]));
        }
        for (uint32_t t = 0; t < total; ++t) {
            hiprz_tri tri{};
            const uint32_t k = seed * 0x10001u + uint32_t(w.tris.size()) * 16u;
            for (int a = 0; a < 3; ++a) tri.v1[a] = coordinate(k + a), tri.v2[a] = coordinate(k + 3 + a), tri.v3[a] = coordinate(k + 6 + a);
            tri.material_flags = 0u, tri.source_index = t;
            w.tris.push_back(tri);
            w.attrs.push_back(hiprz_tri_attr{});
        }
    }
    for (uint32_t i = 0; i < n_inst; ++i) {
        hiprz_instance in{};
        in.blas_root = w.mesh_root[instance_mesh[i]];
        for (int a = 0; a < 3; ++a) in.scale[a] = 1.0f + 0.25f * float(i), in.position[a] = float(i), in.bb_min[a] = -40.0f, in.bb_max[a] = 40.0f;
        in.x_axis[0] = in.y_axis[1] = in.z_axis[2] = 1.0f;
        in.material_base = i, in.material_count = 1u;
        w.instances.push_back(in);
        w.inst_materials.push_back(1);
        w.tlas_order.push_back(i);
    }
    w.materials.assign(2, hiprz_material{});
    for (auto& m : w.materials) m.texture = m.normal_map = m.metalness_map = m.roughness_map = m.emission_map = -1;
    hiprz_scene& sc = w.scene;
    sc.n_nodes = uint32_t(w.nodes.size()), sc.nodes = w.nodes.data(), sc.tlas_root = 0u;
    sc.n_tlas_order = n_inst, sc.tlas_order = w.tlas_order.data();
    sc.n_tris = uint32_t(w.tris.size()), sc.tris = w.tris.data(), sc.tri_attrs = w.attrs.data();
    sc.n_instances = n_inst, sc.instances = w.instances.data();
    sc.n_inst_materials = n_inst, sc.inst_materials = w.inst_materials.data();
    sc.n_materials = 2u, sc.materials = w.materials.data();
}

// every host stage of an upload; `pair_records` as pack_scene takes it
void pack(const World& w, uint32_t tree_mode, bool pair_records, PackedScene& out) {
    SceneCheck chk;
    ChosenTrees trees;
    DerivedTables derived;
    std::string error;
    CHECK(check_scene(&w.scene, chk) == HIPRZ_OK, "%s", chk.error.c_str());
    CHECK(choose_trees(&w.scene, tree_mode, 52u * 1024u, chk, trees, error) == HIPRZ_OK, "%s", error.c_str());
    CHECK(derive_tables(&trees.scene, chk, derived) == HIPRZ_OK, "%s", chk.error.c_str());
    CHECK(pack_scene(trees, std::move(derived), out, error, pair_records) == HIPRZ_OK, "%s", error.c_str());
}

uint16_t half_word(const std::vector<uint8_t>& bytes, size_t at) {
    uint16_t v;
    std::memcpy(&v, bytes.data() + at, 2);
    return v;
}

// The checks of one scene.  `expect_section`: some instance's mesh is one leaf, the world is one leaf of at most 8, the snapshot's trees.
int g_scenes = 0;
void check_world(const char* name, const std::vector<MeshSpec>& meshes, const std::vector<uint32_t>& instance_mesh, bool split_world, uint32_t tree_mode,
                 bool expect_section) {
    World w;
    build(w, meshes, instance_mesh, split_world, uint32_t(g_scenes) + 1u);
    PackedScene with, without;
    pack(w, tree_mode, true, with);
    pack(w, tree_mode, false, without);
    // the blob and its seven offsets do not know about the section
    CHECK(with.blob == without.blob, "%s: the blob differs", name);
    const uint32_t off_with[7] = {with.off_nodes, with.off_tlas_order, with.off_instances, with.off_tris, with.off_tri_attrs, with.off_materials, with.off_inst_materials};
    const uint32_t off_without[7] = {without.off_nodes, without.off_tlas_order, without.off_instances, without.off_tris, without.off_tri_attrs, without.off_materials, without.off_inst_materials};
    for (int k = 0; k < 7; ++k) CHECK(off_with[k] == off_without[k], "%s: offset %d", name, k);
    CHECK(with.blob.size() == with.off_inst_materials + ((4u * w.inst_materials.size() + 15u) & ~size_t(15)), "%s: the blob does not end behind inst_materials", name);
    CHECK(without.pair_section.empty() && without.hot_bytes() == without.blob.size(), "%s: a section that was not asked for", name);
    CHECK(with.hot_bytes() == with.blob.size() + with.pair_section.size(), "%s: total", name);
    CHECK(with.blob.size() % 16u == 0u, "%s: the section would not start 16-byte aligned", name);
    const std::vector<uint8_t>& sec = with.pair_section;
    if (!expect_section) {
        CHECK(sec.empty(), "%s: %zu bytes of section", name, sec.size());
        std::printf("%s: no section, hot buffer %zu bytes\n", name, with.hot_bytes());
        g_scenes += 1;
        return;
    }
    const uint32_t n_inst = uint32_t(instance_mesh.size()), table_bytes = ((n_inst + 3u) & ~3u) * 2u;
    CHECK(with.flat_world, "%s: not a flat world", name);
    CHECK(sec.size() >= table_bytes && sec.size() % 16u == 0u, "%s: %zu bytes", name, sec.size());
    // the records: per single-leaf mesh, in first-use order, ceil(n / 2); the table points every instance at its mesh's first record
    size_t expected_records = 0;
    std::vector<uint32_t> first_of_mesh(meshes.size(), RZ_END);
    for (uint32_t i = 0; i < n_inst; ++i) {
        const uint32_t m = instance_mesh[i], entry = half_word(sec, 2u * i);  // in units of 8 bytes
        if (meshes[m].leaves.size() != 1u) {
            CHECK(entry == kPairNone, "%s: instance %u of a mesh with an inner root has entry %u", name, i, entry);
            continue;
        }
        if (first_of_mesh[m] == RZ_END) {
            first_of_mesh[m] = table_bytes + uint32_t(expected_records) * kPairRecordBytes;
            expected_records += (meshes[m].leaves[0] + 1u) / 2u;
        }
        CHECK(8u * entry == first_of_mesh[m], "%s: instance %u: entry %u, its mesh's records start at byte %u", name, i, entry, first_of_mesh[m]);
        CHECK(8u * entry <= sec.size(), "%s: instance %u: entry %u", name, i, entry);
    }
    for (uint32_t i = n_inst; i < table_bytes / 2u; ++i) CHECK(half_word(sec, 2u * i) == kPairNone, "%s: table padding", name);
    const size_t used = table_bytes + expected_records * kPairRecordBytes;
    CHECK(sec.size() == ((used + 15u) & ~size_t(15)), "%s: %zu bytes for %zu records", name, sec.size(), expected_records);
    for (size_t at = used; at < sec.size(); ++at) CHECK(sec[at] == 0u, "%s: padding behind the records", name);
    // every record against the blob's triangle records (which are v1, v2 - v1, v3 - v1 of the input, checked here as well), bit for bit
    for (size_t m = 0; m < meshes.size(); ++m) {
        if (first_of_mesh[m] == RZ_END) continue;
        const uint32_t n = meshes[m].leaves[0], begin = w.mesh_first_tri[m];
        for (uint32_t p = 0; 2u * p < n; ++p) {
            const size_t rec = first_of_mesh[m] + size_t(p) * kPairRecordBytes;
            for (uint32_t e = 0; e < 2u; ++e) {
                const uint32_t t = begin + 2u * p + ((e == 1u && 2u * p + 1u < n) ? 1u : 0u);  // the b half of an odd leaf's last record repeats a
                hiprz_tri dev;
                std::memcpy(&dev, with.blob.data() + with.off_tris + sizeof(hiprz_tri) * t, sizeof(hiprz_tri));
                const hiprz_tri& src = w.tris[t];
                for (uint32_t a = 0; a < 3u; ++a) {
                    const float edge1 = src.v2[a] - src.v1[a], edge2 = src.v3[a] - src.v1[a];
                    CHECK(std::memcmp(&dev.v1[a], &src.v1[a], 4) == 0 && std::memcmp(&dev.v2[a], &edge1, 4) == 0 && std::memcmp(&dev.v3[a], &edge2, 4) == 0,
                          "%s: blob triangle %u", name, t);
                    CHECK(std::memcmp(sec.data() + rec + 8u * a + 4u * e, &dev.v1[a], 4) == 0, "%s: mesh %zu record %u half %u v1[%u]", name, m, p, e, a);
                    CHECK(std::memcmp(sec.data() + rec + 24u + 8u * a + 4u * e, &dev.v2[a], 4) == 0, "%s: mesh %zu record %u half %u edge1[%u]", name, m, p, e, a);
                    CHECK(std::memcmp(sec.data() + rec + 48u + 8u * a + 4u * e, &dev.v3[a], 4) == 0, "%s: mesh %zu record %u half %u edge2[%u]", name, m, p, e, a);
                }
            }
        }
    }
    std::printf("%s: %zu records, section %zu bytes behind a blob of %zu\n", name, expected_records, sec.size(), with.blob.size());
    g_scenes += 1;
}

}  // namespace

int main() {
    auto one = [](uint32_t n) { return MeshSpec{{n}}; };
    // leaf sizes 1, 2, 3, 4, 5, 8, 9 and a second instance of the first mesh: eight instances, the largest flat world
    check_world("small leaves", {one(1), one(2), one(3), one(4), one(5), one(8), one(9)}, {0, 1, 2, 3, 4, 5, 6, 0}, false, HIPRZ_TREE_REFERENCE, true);
    // 12, 31, 32; the 31 used twice, not by neighbouring instances
    check_world("large leaves", {one(12), one(31), one(32)}, {1, 0, 2, 1}, false, HIPRZ_TREE_REFERENCE, true);
    // a mesh whose root is an inner node between single-leaf neighbours: no record, the neighbours' records follow one another
    check_world("inner root beside leaves", {one(3), MeshSpec{{3, 2}}, one(5)}, {0, 1, 2, 1}, false, HIPRZ_TREE_REFERENCE, true);
    // a leaf of no triangle at all has no record and does not move its neighbour's
    check_world("empty leaf", {one(0), one(2)}, {0, 1}, false, HIPRZ_TREE_REFERENCE, true);
    // three instances: the table is padded to four entries
    check_world("three instances", {one(4)}, {0, 0, 0}, false, HIPRZ_TREE_REFERENCE, true);
    // no section: nine instances in the world's leaf; a world tree that is not one leaf; no single-leaf mesh; trees rebuilt at upload
    check_world("nine instances", {one(2)}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, false, HIPRZ_TREE_REFERENCE, false);
    check_world("split world", {one(2), one(3)}, {0, 1, 0, 1}, true, HIPRZ_TREE_REFERENCE, false);
    check_world("inner roots only", {MeshSpec{{2, 2}}}, {0, 0}, false, HIPRZ_TREE_REFERENCE, false);
    check_world("device trees", {one(12), one(3)}, {0, 1}, false, HIPRZ_TREE_DEVICE, false);
    check_world("surface-area trees", {one(12), one(3)}, {0, 1}, false, HIPRZ_TREE_SAH, false);
    std::printf("pair records: %d scenes ok\n", g_scenes);
    return 0;
}
