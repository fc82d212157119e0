// The packer's surface section (rayzath_amd/csrc/hiprz_scene_host.cpp: pack_surface_section) on the host alone.  tests/test_surface_records.py
// writes scenes into a file, compiles this program with hiprz_scene_host.cpp and hiprz_host.cpp under AddressSanitizer and UBSan, runs it as a
// child process and compares the sections it writes back with a numpy restatement.
// usage: surface_records IN OUT
// IN:  u32 n_scenes, then per scene nine u32 (tree_mode, n_nodes, tlas_root, n_tlas_order, n_tris, n_instances, n_inst_materials, n_materials,
//      0) and the arrays nodes, tlas_order, tris, tri_attrs, instances, inst_materials, materials as the records of include/hiprz.h.
// OUT: per scene four u32 (own_trees, stack_entries, hot_bytes, section bytes) and the section.
// Every scene goes through every host stage of an upload; the program itself checks that the blob, its offsets, the pair section and
// hot_bytes() are what they were before the section was built.  Prints one line per scene and "surface records: N scenes ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiprz_scene_host.hpp"

using namespace hiprz;

namespace {

#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                     \
            std::printf("\n");                                            \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

template <class T>
std::vector<T> read_array(std::FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n) CHECK(std::fread(v.data(), sizeof(T), n, f) == n, "short read");
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    CHECK(argc == 3, "usage: surface_records IN OUT");
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    CHECK(in && out, "cannot open %s / %s", argv[1], argv[2]);
    const uint32_t n_scenes = read_array<uint32_t>(in, 1)[0];
    for (uint32_t k = 0; k < n_scenes; ++k) {
        const std::vector<uint32_t> head = read_array<uint32_t>(in, 9);
        const std::vector<hiprz_node> nodes = read_array<hiprz_node>(in, head[1]);
        const std::vector<uint32_t> tlas_order = read_array<uint32_t>(in, head[3]);
        const std::vector<hiprz_tri> tris = read_array<hiprz_tri>(in, head[4]);
        const std::vector<hiprz_tri_attr> attrs = read_array<hiprz_tri_attr>(in, head[4]);
        const std::vector<hiprz_instance> instances = read_array<hiprz_instance>(in, head[5]);
        const std::vector<int32_t> inst_materials = read_array<int32_t>(in, head[6]);
        const std::vector<hiprz_material> materials = read_array<hiprz_material>(in, head[7]);
        hiprz_scene sc{};
        sc.n_nodes = head[1], sc.nodes = nodes.data(), sc.tlas_root = head[2];
        sc.n_tlas_order = head[3], sc.tlas_order = tlas_order.data();
        sc.n_tris = head[4], sc.tris = tris.data(), sc.tri_attrs = attrs.data();
        sc.n_instances = head[5], sc.instances = instances.data();
        sc.n_inst_materials = head[6], sc.inst_materials = inst_materials.data();
        sc.n_materials = head[7], sc.materials = materials.data();

        SceneCheck chk;
        ChosenTrees trees;
        DerivedTables derived;
        PackedScene packed;
        std::string error;
        CHECK(check_scene(&sc, chk) == HIPRZ_OK, "scene %u: %s", k, chk.error.c_str());
        CHECK(choose_trees(&sc, head[0], 52u * 1024u, chk, trees, error) == HIPRZ_OK, "scene %u: %s", k, error.c_str());
        CHECK(derive_tables(&trees.scene, chk, derived) == HIPRZ_OK, "scene %u: %s", k, chk.error.c_str());
        CHECK(pack_scene(trees, std::move(derived), packed, error) == HIPRZ_OK, "scene %u: %s", k, error.c_str());
        const std::vector<uint8_t> blob = packed.blob, pairs = packed.pair_section;
        const size_t hot_bytes = packed.hot_bytes();
        const uint32_t off[7] = {packed.off_nodes, packed.off_tlas_order, packed.off_instances, packed.off_tris, packed.off_tri_attrs, packed.off_materials, packed.off_inst_materials};
        const uint32_t stack_entries = chk.world_depth + chk.mesh_depth + 2u;
        const std::vector<uint8_t> section = pack_surface_section(trees, packed, stack_entries, 160u * 1024u);
        // the blob, its offsets, the pair section and the staged total do not know about the section
        CHECK(packed.blob == blob && packed.pair_section == pairs && packed.hot_bytes() == hot_bytes, "scene %u: the hot buffer changed", k);
        const uint32_t off_after[7] = {packed.off_nodes, packed.off_tlas_order, packed.off_instances, packed.off_tris, packed.off_tri_attrs, packed.off_materials, packed.off_inst_materials};
        CHECK(std::memcmp(off, off_after, sizeof off) == 0 && hot_bytes == blob.size() + pairs.size(), "scene %u: offsets", k);
        CHECK(section.size() % 16u == 0u, "scene %u: %zu bytes", k, section.size());
        // a scene that could not be staged has none
        CHECK(pack_surface_section(trees, packed, stack_entries, hot_bytes + size_t(stack_entries) * 1024u - 1u).empty(), "scene %u: a section beyond the limit", k);
        const uint32_t result[4] = {trees.own_trees ? 1u : 0u, stack_entries, uint32_t(hot_bytes), uint32_t(section.size())};
        CHECK(std::fwrite(result, 4, 4, out) == 4, "write");
        if (!section.empty()) CHECK(std::fwrite(section.data(), 1, section.size(), out) == section.size(), "write");
        std::printf("scene %u: %u instances, %u triangles, hot buffer %zu bytes unchanged, section %zu bytes\n", k, sc.n_instances, sc.n_tris, hot_bytes, section.size());
    }
    CHECK(std::fclose(out) == 0, "close");
    std::fclose(in);
    std::printf("surface records: %u scenes ok\n", n_scenes);
    return 0;
}
