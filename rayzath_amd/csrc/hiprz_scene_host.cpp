// hiprz_scene_host.cpp — see hiprz_scene_host.hpp: scene validation, the derived walk tables and the device layout of every scene
// record, on the host alone (no HIP header).
#include "hiprz_scene_host.hpp"

#include <algorithm>
#include <cmath>

namespace hiprz {

namespace {
struct TreeCheck {
    const hiprz_scene* sc;
    std::vector<uint32_t>& skip;
    std::vector<uint8_t> visited;
    uint32_t max_depth = 0;
    std::string error;
    std::vector<uint32_t> world_leaves;

    // Walks one tree from `root`, verifies every index it will make the kernel follow, fills
    // the skip links, returns false on the first violation.  `is_world`: leaves index tlas_order.
    bool walk(uint32_t root, bool is_world) {
        struct Item {
            uint32_t node, skip, depth;
        };
        std::vector<Item> stack{{root, RZ_END, 1u}};
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            if (it.node >= sc->n_nodes) return err("node index out of range");
            if (visited[it.node]) return err("node reachable twice (trees must be disjoint and acyclic)");
            visited[it.node] = 1;
            skip[it.node] = it.skip;
            if (it.depth > max_depth) max_depth = it.depth;
            if (it.depth > 64u) return err("tree deeper than 64 levels");
            const hiprz_node& n = sc->nodes[it.node];
            if (n.meta & HIPRZ_NODE_LEAF) {
                const uint64_t end = uint64_t(n.begin) + (n.meta & HIPRZ_NODE_COUNT_MASK);
                if (end > (is_world ? sc->n_tlas_order : sc->n_tris)) return err("leaf range out of bounds");
                if (is_world) world_leaves.push_back(it.node);
            } else {
                if (uint64_t(n.begin) + 1 >= sc->n_nodes) return err("child index out of range");
                stack.push_back({n.begin + 1, it.skip, it.depth + 1});
                stack.push_back({n.begin, n.begin + 1, it.depth + 1});
            }
        }
        return true;
    }
    bool err(const char* m) {
        error = m;
        return false;
    }
};
}  // namespace

bool material_maps_ok(const hiprz_material& m, const hiprz_texture* textures, uint32_t n_textures) {
    auto tex_ok = [&](int32_t t, uint32_t kind) { return t < 0 || (uint32_t(t) < n_textures && textures[t].kind == kind); };
    return tex_ok(m.texture, HIPRZ_TEX_RGBA8) && tex_ok(m.normal_map, HIPRZ_TEX_RGBA8) && tex_ok(m.metalness_map, HIPRZ_TEX_R8) &&
           tex_ok(m.roughness_map, HIPRZ_TEX_R8) && tex_ok(m.emission_map, HIPRZ_TEX_R32F);
}

int check_scene(const hiprz_scene* sc, SceneCheck& out) {
    auto bad = [&out](const std::string& m) {
        out.error = m;
        return HIPRZ_ERR_INVALID;
    };
    if (!sc) return bad("scene is null");
    // ---- validate everything the kernels will dereference, on the host, before any launch ----
    if (sc->n_materials < 2 || !sc->materials) return bad("scene needs materials[0]=world, [1]=default");
    if (sc->n_materials > 65536u) return bad("more than 65536 materials");
    if ((sc->n_nodes && !sc->nodes) || (sc->n_tris && (!sc->tris || !sc->tri_attrs)) || (sc->n_instances && !sc->instances) ||
        (sc->n_tlas_order && !sc->tlas_order) || (sc->n_inst_materials && !sc->inst_materials) ||
        (sc->n_textures && !sc->textures) || (sc->texel_bytes && !sc->texels) || (sc->n_spot_lights && !sc->spot_lights) ||
        (sc->n_direct_lights && !sc->direct_lights))
        return bad("upload_scene: null array with non-zero count");
    for (uint32_t i = 0; i < sc->n_textures; ++i) {
        const hiprz_texture& t = sc->textures[i];
        const uint64_t texel = t.kind == HIPRZ_TEX_R8 ? 1u : 4u;
        if (t.kind > HIPRZ_TEX_R32F || t.width == 0 || t.height == 0 || (t.offset & 3u) ||
            uint64_t(t.offset) + texel * t.width * t.height > sc->texel_bytes)
            return bad("texture " + std::to_string(i) + ": bad kind/size/offset");
    }
    for (uint32_t i = 0; i < sc->n_materials; ++i)
        if (!material_maps_ok(sc->materials[i], sc->textures, sc->n_textures)) return bad("material " + std::to_string(i) + ": map index/kind invalid");
    for (uint32_t i = 0; i < sc->n_inst_materials; ++i)
        if (sc->inst_materials[i] >= int32_t(sc->n_materials))
            return bad("inst_materials[" + std::to_string(i) + "] out of range");
    for (uint32_t i = 0; i < sc->n_tlas_order; ++i)
        if (sc->tlas_order[i] >= sc->n_instances) return bad("tlas_order entry out of range");
    for (uint32_t i = 0; i < sc->n_instances; ++i) {
        const hiprz_instance& in = sc->instances[i];
        if (in.material_count > 64u || uint64_t(in.material_base) + in.material_count > sc->n_inst_materials)
            return bad("instance " + std::to_string(i) + ": material table out of range");
    }
    std::vector<uint32_t> skip(sc->n_nodes ? sc->n_nodes : 1, RZ_END);
    TreeCheck check{sc, skip, std::vector<uint8_t>(sc->n_nodes ? sc->n_nodes : 1, 0)};
    uint32_t world_depth = 0, mesh_depth = 0;
    if (sc->n_instances) {
        if (!check.walk(sc->tlas_root, true)) return bad("world tree: " + check.error);
        world_depth = check.max_depth;
        std::vector<uint8_t> root_seen(sc->n_nodes, 0);
        for (uint32_t i = 0; i < sc->n_tlas_order; ++i) {
            const uint32_t root = sc->instances[sc->tlas_order[i]].blas_root;
            if (root >= sc->n_nodes) return bad("instance mesh root out of range");
            if (root_seen[root]) continue;
            root_seen[root] = 1;
            check.max_depth = 0;
            if (!check.walk(root, false)) return bad("mesh tree: " + check.error);
            mesh_depth = std::max(mesh_depth, check.max_depth);
        }
    }
    out.skip = std::move(skip);
    out.reachable = std::move(check.visited);
    out.world_leaves = std::move(check.world_leaves);
    out.world_depth = world_depth, out.mesh_depth = mesh_depth;
    return HIPRZ_OK;
}

int derive_tables(const hiprz_scene* sc, SceneCheck& chk, DerivedTables& out) {
    // Relayout: breadth-first over ALL trees at once (world root, then every distinct mesh root, then their child
    // pairs, ...), children staying adjacent.  The levels nearest the roots become a prefix of the array (the part
    // MODE 3 caches in LDS) and siblings/cousins share cache lines.  Leaf ranges are untouched.
    std::vector<uint32_t>& new_index = out.new_index;
    new_index.assign(sc->n_nodes, RZ_END);
    std::vector<uint32_t> bfs;
    bfs.reserve(sc->n_nodes);
    auto enqueue = [&](uint32_t old) {
        if (old < sc->n_nodes && new_index[old] == RZ_END) {
            new_index[old] = uint32_t(bfs.size());
            bfs.push_back(old);
        }
    };
    if (sc->n_instances) enqueue(sc->tlas_root);
    for (uint32_t i = 0; i < sc->n_tlas_order; ++i) enqueue(sc->instances[sc->tlas_order[i]].blas_root);
    // Child pairs follow the roots.  A 64-byte record pair is one 128-byte cache line when it starts at an even index: one empty slot
    // behind an odd number of roots puts every pair on a line of its own, so that the second child — visited after the first one's
    // subtree, or probed together with it — is on the line the first one brought in.
    const uint32_t pad_at = (bfs.size() & 1u) ? uint32_t(bfs.size()) : RZ_END;
    if (pad_at != RZ_END) bfs.push_back(RZ_END);
    for (size_t q = 0; q < bfs.size(); ++q) {
        if (bfs[q] == RZ_END) continue;
        const hiprz_node& n = sc->nodes[bfs[q]];
        if (!(n.meta & HIPRZ_NODE_LEAF)) enqueue(n.begin), enqueue(n.begin + 1);
    }
    for (uint32_t old = 0; old < sc->n_nodes; ++old) enqueue(old);  // nodes no instance reaches keep a slot
    const size_t n_total = bfs.size();  // the scene's nodes + the padding slot
    std::vector<hiprz_node>& dnodes = out.dnodes;
    std::vector<uint32_t>& dskip = out.dskip;
    hiprz_node empty{};
    empty.meta = HIPRZ_NODE_LEAF;  // no triangles, reached by nothing
    dnodes.assign(n_total ? n_total : 0, empty);
    dskip.assign(n_total ? n_total : 1, RZ_END);
    for (uint32_t old = 0; old < sc->n_nodes; ++old) {
        hiprz_node n = sc->nodes[old];
        if (!(n.meta & HIPRZ_NODE_LEAF)) n.begin = new_index[n.begin];
        dnodes[new_index[old]] = n;
        dskip[new_index[old]] = chk.skip[old] == RZ_END ? RZ_END : new_index[chk.skip[old]];
    }

    // ---- skip links per ray octant (front-to-back walk) ----
    // Under octant o an inner node with partition type p (X=2, Y=1, Z=0) is left towards its SECOND child first when bit p of o is
    // set; a size split (type 3) is never flipped.  The child visited first links to its sibling, the other one inherits the
    // parent's link.  Parents precede their children in the breadth-first numbering, so one ascending sweep fills all tables;
    // roots end their walks (RZ_END).  Octant 0 reproduces dskip.
    std::vector<uint32_t>& dskip8 = out.dskip8;
    dskip8.assign((n_total ? n_total : 1) * 8u, RZ_END);
    for (uint32_t n = 0; n < n_total; ++n) {
        const hiprz_node& nd = dnodes[n];
        if (nd.meta & HIPRZ_NODE_LEAF) continue;
        const uint32_t ptype = (nd.meta >> HIPRZ_NODE_PTYPE_SHIFT) & 3u, c0 = nd.begin;
        if (c0 <= n || size_t(c0) + 1 >= n_total) continue;  // cannot happen after check_scene + the BFS relayout; keeps the sweep safe
        for (uint32_t o = 0; o < 8u; ++o) {
            const uint32_t flip = (o >> ptype) & 1u;  // ptype 3 reads bit 3 = 0
            dskip8[size_t(c0 + flip) * 8u + o] = c0 + 1u - flip;
            dskip8[size_t(c0 + 1u - flip) * 8u + o] = dskip8[size_t(n) * 8u + o];
        }
    }

    // The kernels follow these derived tables blindly: prove on the host that every walk over them terminates
    // (each step moves strictly forward in depth-first order, so a walk may take at most one step per node).
    {
        auto terminates = [](const std::vector<hiprz_node>& nodes, const std::vector<uint32_t>& links, uint32_t root) {
            uint32_t n = root;
            for (size_t steps = 0; steps <= nodes.size(); ++steps) {
                if (n == RZ_END) return true;
                if (n >= nodes.size()) return false;
                const hiprz_node& nd = nodes[n];
                n = !(nd.meta & HIPRZ_NODE_LEAF) ? nd.begin : links[n];
            }
            return false;
        };
        bool ok = true;
        for (uint32_t old = 0; ok && old < sc->n_nodes; ++old)  // the stack walks reach the second child as first + 1
            if (!(sc->nodes[old].meta & HIPRZ_NODE_LEAF)) ok = new_index[sc->nodes[old].begin + 1] == new_index[sc->nodes[old].begin] + 1u;
        if (ok && sc->n_instances) ok = terminates(dnodes, dskip, new_index[sc->tlas_root]);
        for (uint32_t i = 0; ok && i < sc->n_tlas_order; ++i) {
            const uint32_t root = new_index[sc->instances[sc->tlas_order[i]].blas_root];
            ok = terminates(dnodes, dskip, root);
        }
        // the same for every octant's links: a walk that enters every box takes exactly one step per node of the tree it walks
        auto terminates8 = [&](uint32_t root, uint32_t o) {
            uint32_t n = root;
            for (size_t steps = 0; steps <= dnodes.size(); ++steps) {
                if (n == RZ_END) return true;
                if (n >= dnodes.size()) return false;
                const hiprz_node& nd = dnodes[n];
                if (!(nd.meta & HIPRZ_NODE_LEAF)) n = nd.begin + ((o >> ((nd.meta >> HIPRZ_NODE_PTYPE_SHIFT) & 3u)) & 1u);
                else n = dskip8[size_t(n) * 8u + o];
            }
            return false;
        };
        for (uint32_t old = 0; ok && old < sc->n_nodes; ++old)  // octant 0 is the reference's order (nodes no walk reaches have no links to compare)
            if (old < chk.reachable.size() && chk.reachable[old]) ok = dskip8[size_t(new_index[old]) * 8u] == dskip[new_index[old]];
        if (ok && sc->n_instances) ok = terminates8(new_index[sc->tlas_root], 0u);
        {
            std::vector<uint8_t> seen(n_total ? n_total : 1, 0);
            for (uint32_t i = 0; ok && i < sc->n_tlas_order; ++i) {
                const uint32_t root = new_index[sc->instances[sc->tlas_order[i]].blas_root];
                if (seen[root]) continue;
                seen[root] = 1;
                for (uint32_t o = 0; ok && o < 8u; ++o) ok = terminates8(root, o);
            }
        }
        if (!ok) {
            chk.error = "internal: derived walk tables are inconsistent (refusing to launch)";
            return HIPRZ_ERR_INVALID;
        }
    }
    return HIPRZ_OK;
}

uint32_t device_build_regions(std::vector<DeviceMesh>& meshes, uint32_t first_free_slot) {
    uint32_t cursor = first_free_slot;
    for (auto& m : meshes) {
        if (m.n_tris <= kLeafMax) {
            m.region = RZ_END;  // stays the single leaf of the uploaded placeholder
            continue;
        }
        if (!(cursor & 1u)) cursor += 1u;
        m.region = cursor;
        cursor += 2u * m.n_tris - 1u;
    }
    return cursor;
}

int choose_trees(const hiprz_scene* sc, uint32_t tree_mode, size_t lds_limit, SceneCheck& chk, ChosenTrees& out, std::string& error) {
    out.scene = *sc;
    uint32_t tree = tree_mode;
    if (tree == HIPRZ_TREE_AUTO) {
        // a scene whose records can be staged in LDS keeps the snapshot's trees (the resident kernels walk those); any other gets the
        // device's surface-area trees.  (A lower bound of the hot blob: node records, triangles + shading records, instances.)
        const size_t records = size_t(sc->n_nodes) * 32u + size_t(sc->n_tris) * 144u + size_t(sc->n_instances) * 112u;
        tree = records > lds_limit ? HIPRZ_TREE_DEVICE : HIPRZ_TREE_REFERENCE;
    }
    if (tree == HIPRZ_TREE_REFERENCE || sc->n_tris == 0u) return HIPRZ_OK;
    const uint32_t max_nodes = sc->n_nodes + 2u * sc->n_tris + sc->n_instances + 1u;
    std::vector<uint32_t> order(sc->n_tris), roots(sc->n_instances ? sc->n_instances : 1u);
    uint32_t n_nodes = 0u, tlas_root = 0u;
    out.nodes.resize(max_nodes);
    if (hiprz_rebuild_mesh_trees(sc, tree, out.nodes.data(), max_nodes, &n_nodes, order.data(), roots.data(), &tlas_root) != HIPRZ_OK) {
        if (tree_mode == HIPRZ_TREE_AUTO) return HIPRZ_OK;  // HIPRZ_TREE_AUTO promises an upload wherever the snapshot's own trees are valid
        error = "upload_scene: the mesh trees could not be rebuilt (leaves of a mesh must tile one range of triangles)";
        return HIPRZ_ERR_INVALID;
    }
    out.nodes.resize(n_nodes);
    // (the placeholder trees of a device build keep the snapshot's order when its meshes lie in first-use order, as the hosts'
    // flatteners lay them out: then the 144 bytes per triangle are not copied, and position i is what triangle i is ranked by)
    out.identity_order = true;
    for (uint32_t i = 0; i < sc->n_tris && out.identity_order; ++i) out.identity_order = order[i] == i;
    if (!out.identity_order) {
        out.tris.resize(sc->n_tris), out.attrs.resize(sc->n_tris);
        for (uint32_t i = 0; i < sc->n_tris; ++i) {
            out.tris[i] = sc->tris[order[i]];
            out.tris[i].pad0 = order[i];
            out.attrs[i] = sc->tri_attrs[order[i]];
        }
        out.scene.tris = out.tris.data(), out.scene.tri_attrs = out.attrs.data();
    }
    out.instances.assign(sc->instances, sc->instances + sc->n_instances);
    for (uint32_t i = 0; i < sc->n_instances; ++i) out.instances[i].blas_root = roots[i];
    out.scene.n_nodes = n_nodes, out.scene.nodes = out.nodes.data(), out.scene.tlas_root = tlas_root;
    out.scene.instances = out.instances.data();
    out.tree = tree, out.own_trees = true;
    if (check_scene(&out.scene, chk) != HIPRZ_OK) {
        error = "upload_scene: rebuilt trees: " + chk.error;
        return HIPRZ_ERR_INVALID;
    }
    return HIPRZ_OK;
}

int pack_scene(const ChosenTrees& trees, DerivedTables&& derived, PackedScene& out, std::string& error, bool pair_records) {
    const hiprz_scene* sc = &trees.scene;
    out.new_index = std::move(derived.new_index), out.nodes = std::move(derived.dnodes), out.skip = std::move(derived.dskip);
    const std::vector<uint32_t>& new_index = out.new_index;
    std::vector<hiprz_node>& dnodes = out.nodes;
    out.fast_div = true;
    for (const auto& n : dnodes)
        for (int a = 0; a < 3; ++a) out.fast_div = out.fast_div && coord_ok(n.bb_min[a]) && coord_ok(n.bb_max[a]);
    for (uint32_t i = 0; i < sc->n_instances; ++i)
        for (int a = 0; a < 3; ++a) out.fast_div = out.fast_div && coord_ok(sc->instances[i].bb_min[a]) && coord_ok(sc->instances[i].bb_max[a]);
    for (auto& n : dnodes) interleave_box(n);
    out.instances.assign(sc->instances, sc->instances + sc->n_instances);
    for (uint32_t i = 0; i < sc->n_instances; ++i) {
        hiprz_instance& in = out.instances[i];
        if (in.blas_root < sc->n_nodes) in.blas_root = new_index[in.blas_root];
        pack_instance_placement(in, sc->instances[i]);
    }
    std::vector<uint8_t>& blob = out.blob;
    blob.clear();
    auto append = [&blob](const void* src, size_t bytes) {
        const uint32_t off = uint32_t(blob.size());
        blob.resize(blob.size() + ((bytes + 15u) & ~size_t(15)), 0);
        if (bytes) std::memcpy(blob.data() + off, src, bytes);
        return off;
    };
    out.off_nodes = append(dnodes.data(), sizeof(hiprz_node) * dnodes.size());
    out.off_tlas_order = append(sc->tlas_order, sizeof(uint32_t) * sc->n_tlas_order);
    out.off_instances = append(out.instances.data(), sizeof(hiprz_instance) * out.instances.size());
    {   // device triangles hold v1 and the edges v2 - v1, v3 - v1; v2 and v3 themselves (normal mapping only) move into
        // the padding words of the attribute record
        std::vector<hiprz_tri> dtris(sc->tris, sc->tris + sc->n_tris);
        std::vector<hiprz_tri_attr> dattrs(sc->tri_attrs, sc->tri_attrs + sc->n_tris);
        for (uint32_t i = 0; i < sc->n_tris; ++i) {
            hiprz_tri& t = dtris[i];
            hiprz_tri_attr& a = dattrs[i];
            if (!trees.own_trees || trees.identity_order) t.pad0 = i;  // position in the reference's leaf order: what equally distant hits are ranked by
            a.pad0 = t.v2[0], a.pad1 = t.v2[1], a.pad2 = t.v2[2], a.pad3 = t.v3[0], a.pad4[0] = t.v3[1], a.pad4[1] = t.v3[2];
            for (int k = 0; k < 3; ++k) {
                const float v2 = t.v2[k], v3 = t.v3[k];
                t.v2[k] = v2 - t.v1[k];
                t.v3[k] = v3 - t.v1[k];
            }
        }
        out.off_tris = append(dtris.data(), sizeof(hiprz_tri) * dtris.size());
        out.off_tri_attrs = append(dattrs.data(), sizeof(hiprz_tri_attr) * dattrs.size());
    }
    out.off_materials = append(sc->materials, sizeof(hiprz_material) * sc->n_materials);
    out.off_inst_materials = append(sc->inst_materials, sizeof(int32_t) * sc->n_inst_materials);
    if (blob.size() > 0xFFFFFFF0ull) {
        error = "scene geometry exceeds 4 GiB";
        return HIPRZ_ERR_INVALID;
    }

    out.device_meshes.clear();
    out.instance_mesh.assign(sc->n_instances, RZ_END);
    out.node_capacity = uint32_t(dnodes.size()), out.world_region = 0u;
    if (trees.device_trees()) {
        std::vector<uint32_t> mesh_of_root(sc->n_nodes, RZ_END);
        for (uint32_t i = 0; i < sc->n_instances; ++i) {
            const uint32_t root = sc->instances[i].blas_root;
            if (root >= sc->n_nodes) continue;
            if (mesh_of_root[root] == RZ_END) {
                const hiprz_node& leaf = sc->nodes[root];  // the placeholder of hiprz_rebuild_mesh_trees(.., HIPRZ_TREE_DEVICE, ..): one leaf per mesh
                DeviceMesh m;
                m.tri_first = leaf.begin, m.n_tris = leaf.meta & HIPRZ_NODE_COUNT_MASK;
                m.ref_first = m.n_tris ? (trees.identity_order ? leaf.begin : sc->tris[leaf.begin].pad0) : 0u;
                m.leaf_slot = new_index[root];
                std::memcpy(m.bb_min, leaf.bb_min, 12), std::memcpy(m.bb_max, leaf.bb_max, 12);
                mesh_of_root[root] = uint32_t(out.device_meshes.size());
                out.device_meshes.push_back(m);
            }
            out.instance_mesh[i] = mesh_of_root[root];
        }
        uint32_t cursor = uint32_t(dnodes.size());
        if (!(cursor & 1u)) cursor += 1u;
        out.world_region = cursor;
        cursor += 2u * sc->n_instances + 1u;
        out.node_capacity = device_build_regions(out.device_meshes, cursor);
        out.skip.resize(out.node_capacity, RZ_END);
    }
    out.nodes64.assign(size_t(out.node_capacity ? out.node_capacity : 1) * 16u, RZ_END);
    for (size_t n = 0; n < dnodes.size(); ++n) {
        std::memcpy(&out.nodes64[n * 16u], &dnodes[n], sizeof(hiprz_node));
        std::memcpy(&out.nodes64[n * 16u + 8u], &derived.dskip8[n * 8u], 32);
    }

    out.tlas_root = sc->n_instances ? new_index[sc->tlas_root] : 0u;
    for (int a = 0; a < 3; ++a) {
        const float lo = sc->n_instances ? sc->nodes[sc->tlas_root].bb_min[a] : 0.0f, hi = sc->n_instances ? sc->nodes[sc->tlas_root].bb_max[a] : 0.0f;
        out.bounds_min[a] = lo;
        out.bounds_scale[a] = hi > lo ? 32.0f / (hi - lo) : 0.0f;
    }
    out.flat_world = sc->n_instances != 0u && (sc->nodes[sc->tlas_root].meta & HIPRZ_NODE_LEAF) && (sc->nodes[sc->tlas_root].meta & HIPRZ_NODE_COUNT_MASK) <= 8u;
    // the pair records of the single-leaf meshes (hiprz_scene_host.hpp: PackedScene::pair_section), copied from the blob's triangle records
    out.pair_section.clear();
    if (pair_records && out.flat_world && !trees.own_trees) {
        const uint32_t table_bytes = ((sc->n_instances + 3u) & ~3u) * 2u;
        std::vector<uint16_t> table(table_bytes / 2u, kPairNone);
        std::vector<uint32_t> first_of_root(sc->n_nodes, RZ_END);
        std::vector<uint8_t> records;
        bool any = false;
        for (uint32_t i = 0; i < sc->n_instances; ++i) {
            const uint32_t root = sc->instances[i].blas_root;
            if (root >= sc->n_nodes || !(sc->nodes[root].meta & HIPRZ_NODE_LEAF)) continue;
            if (first_of_root[root] == RZ_END) {
                first_of_root[root] = (table_bytes + uint32_t(records.size())) / 8u;
                const uint32_t begin = sc->nodes[root].begin, n = sc->nodes[root].meta & HIPRZ_NODE_COUNT_MASK;
                for (uint32_t p = 0; 2u * p < n && records.size() < kPairSectionLimit; ++p) {
                    hiprz_tri ab[2];
                    std::memcpy(&ab[0], blob.data() + out.off_tris + sizeof(hiprz_tri) * (begin + 2u * p), sizeof(hiprz_tri));
                    ab[1] = ab[0];  // an odd leaf's last record repeats a in b
                    if (2u * p + 1u < n) std::memcpy(&ab[1], blob.data() + out.off_tris + sizeof(hiprz_tri) * (begin + 2u * p + 1u), sizeof(hiprz_tri));
                    float rec[kPairRecordBytes / 4u];
                    for (int k = 0; k < 3; ++k)
                        for (int e = 0; e < 2; ++e) rec[2 * k + e] = ab[e].v1[k], rec[6 + 2 * k + e] = ab[e].v2[k], rec[12 + 2 * k + e] = ab[e].v3[k];
                    const size_t at = records.size();
                    records.resize(at + kPairRecordBytes);
                    std::memcpy(records.data() + at, rec, kPairRecordBytes);
                }
            }
            table[i] = uint16_t(first_of_root[root]), any = true;
        }
        // (beyond the limit a table entry could not say where a mesh's records start: no section — the blob of such a scene, 144 bytes
        // per triangle against the section's 36, is far beyond what any kernel stages in LDS, and only staged scenes are read through it)
        if (any && table_bytes + records.size() <= kPairSectionLimit) {
            out.pair_section.assign((table_bytes + records.size() + 15u) & ~size_t(15), 0);
            std::memcpy(out.pair_section.data(), table.data(), table_bytes);
            if (!records.empty()) std::memcpy(out.pair_section.data() + table_bytes, records.data(), records.size());
        }
        if (out.hot_bytes() > 0xFFFFFFF0ull) {
            error = "scene geometry exceeds 4 GiB";
            return HIPRZ_ERR_INVALID;
        }
    }
    std::vector<uint8_t> member(sc->n_instances ? sc->n_instances : 1u, 0);
    for (uint32_t k = 0; k < sc->n_tlas_order; ++k)
        if (sc->tlas_order[k] < sc->n_instances) member[sc->tlas_order[k]] = 1;
    out.world_members.clear();
    for (uint32_t i = 0; i < sc->n_instances; ++i)
        if (member[i]) out.world_members.push_back(i);
    return HIPRZ_OK;
}

namespace {

// fp32 arithmetic of one surface record, every operation rounded on its own as the device rounds it (hiprz_device.hpp: v3 operators,
// transform_forward, normalized); `bad` collects whether any value that went in or came out was subnormal, infinite or NaN
struct SurfaceMath {
    bool bad = false;
    float see(float x) {
        uint32_t b;
        std::memcpy(&b, &x, 4);
        const uint32_t e = (b >> 23) & 0xFFu;
        if (e == 0xFFu || (e == 0u && (b & 0x007FFFFFu) != 0u)) bad = true;
        return x;
    }
    void scaled(const float v[3], float s, float out[3]) {
        for (int a = 0; a < 3; ++a) out[a] = see(v[a] * s);
    }
    void divided(const float v[3], const float d[3], float out[3]) {
        for (int a = 0; a < 3; ++a) out[a] = see(v[a] / d[a]);
    }
    void forward(const hiprz_instance& in, const float v[3], float out[3]) {  // (xa * v.x + ya * v.y) + za * v.z
        for (int a = 0; a < 3; ++a) {
            const float x = see(in.x_axis[a] * v[0]), y = see(in.y_axis[a] * v[1]), z = see(in.z_axis[a] * v[2]);
            out[a] = see(see(x + y) + z);
        }
    }
    void normalize(const float v[3], float out[3]) {  // v * (1 / sqrt((x x + y y) + z z))
        const float xx = see(v[0] * v[0]), yy = see(v[1] * v[1]), zz = see(v[2] * v[2]);
        const float r = see(1.0f / see(std::sqrt(see(see(xx + yy) + zz))));
        scaled(v, r, out);
    }
};

}  // namespace

std::vector<uint8_t> pack_surface_section(const ChosenTrees& trees, const PackedScene& packed, uint32_t stack_entries, size_t lds_limit) {
    std::vector<uint8_t> section;
    const hiprz_scene* sc = &trees.scene;
    if (trees.own_trees || sc->n_instances == 0u || packed.hot_bytes() + size_t(stack_entries) * 1024u > lds_limit) return section;
    // the triangles of a mesh: what the leaves under its root cover (the snapshot was validated: every tree ends)
    struct Range {
        uint32_t lo = RZ_END, hi = 0u;
    };
    std::vector<Range> range_of_root(sc->n_nodes);
    std::vector<uint8_t> ranged(sc->n_nodes, 0);
    const uint32_t table_words = (sc->n_instances + 3u) & ~3u;
    std::vector<uint32_t> table(table_words, 0u);
    std::vector<uint32_t> words;  // the records, 8 words each
    std::vector<uint32_t> todo;
    for (const uint32_t i : packed.world_members) {  // (an instance outside the world tree is never hit, and nobody validated its mesh tree)
        const hiprz_instance& in = sc->instances[i];
        const uint32_t root = in.blas_root;
        if (!ranged[root]) {
            Range r;
            todo.assign(1, root);
            while (!todo.empty()) {
                const hiprz_node& n = sc->nodes[todo.back()];
                todo.pop_back();
                if (n.meta & HIPRZ_NODE_LEAF) {
                    const uint32_t count = n.meta & HIPRZ_NODE_COUNT_MASK;
                    if (count) r.lo = std::min(r.lo, n.begin), r.hi = std::max(r.hi, n.begin + count);
                } else {
                    todo.push_back(n.begin), todo.push_back(n.begin + 1u);
                }
            }
            range_of_root[root] = r, ranged[root] = 1;
        }
        const Range r = range_of_root[root];
        if (r.lo >= r.hi) continue;  // an empty mesh: never hit
        table[i] = uint32_t(words.size() / 16u) - r.lo;  // (modulo 2^32, like the device's addition)
        float scale_in[3];
        SurfaceMath placement;
        for (int a = 0; a < 3; ++a) scale_in[a] = placement.see(in.scale[a]), placement.see(in.x_axis[a]), placement.see(in.y_axis[a]), placement.see(in.z_axis[a]);
        for (uint32_t t = r.lo; t < r.hi; ++t) {
            const uint32_t flags = sc->tris[t].material_flags;
            uint32_t slot = flags & HIPRZ_TRI_MATERIAL_MASK;
            if (slot > 63u) slot = 63u;
            int32_t mat = -1;
            if (slot < in.material_count && uint64_t(in.material_base) + slot < sc->n_inst_materials) mat = sc->inst_materials[in.material_base + slot];
            const uint32_t surface_material = mat < 0 ? HIPRZ_MATERIAL_DEFAULT : uint32_t(mat);
            const float* face_normal = sc->tri_attrs[t].face_normal;
            for (uint32_t external = 0; external < 2u; ++external) {
                const float ef = float(external) * 2.0f - 1.0f;
                SurfaceMath math = placement;
                for (int a = 0; a < 3; ++a) math.see(face_normal[a]);
                float v[3], w[3], normal[3], mapped[3];
                math.scaled(face_normal, ef, v);   // sf.normal = normalized(transform_forward((face_normal * ef) / scale))
                math.divided(v, scale_in, w);
                math.forward(in, w, v);
                math.normalize(v, normal);
                math.divided(face_normal, scale_in, w);  // sf.mapped_normal = normalized(transform_forward(face_normal / scale)) * ef
                math.forward(in, w, v);
                math.normalize(v, w);
                math.scaled(w, ef, mapped);
                uint32_t valid = 0u;
                if (!math.bad) valid = kSurfaceNormalValid | ((flags & HIPRZ_TRI_HAS_NORMALS) ? 0u : kSurfaceMappedValid);
                uint32_t rec[8];
                std::memcpy(rec, normal, 12), std::memcpy(rec + 4, mapped, 12);
                rec[3] = surface_material, rec[7] = valid;
                words.insert(words.end(), rec, rec + 8);
            }
        }
    }
    static_assert(kSurfaceRecordBytes == 32u, "two float4 per record");
    section.resize(4u * (size_t(table_words) + words.size()));
    std::memcpy(section.data(), table.data(), 4u * size_t(table_words));
    if (!words.empty()) std::memcpy(section.data() + 4u * size_t(table_words), words.data(), 4u * words.size());
    return section;
}

uint32_t enter_device_roots(std::vector<hiprz_instance>& instances, const std::vector<uint32_t>& instance_mesh, const std::vector<DeviceMesh>& meshes,
                            uint32_t world_slots) {
    for (size_t i = 0; i < instances.size(); ++i)
        if (instance_mesh[i] != RZ_END && meshes[instance_mesh[i]].region != RZ_END) instances[i].blas_root = meshes[instance_mesh[i]].region;
    uint32_t emitted = world_slots;
    for (const auto& m : meshes) emitted += m.n_slots;
    return emitted;
}

// anyIntersection's answer does not depend on the order in which a ray meets the instances, so the wave-level shadow walk
// (any_hit_packet) need not follow the reference's world tree — built for another purpose: leaves of several instances, met in one fixed
// sequence — and takes a binned-free surface-area tree over the instances' world boxes instead: binary, one instance per leaf, the leaf's
// box being the instance's own (interleaved) box bit for bit, so that the leaf's test is the instance's test.  n log^2 n for n
// instances, 64-byte walk records with the octant-0 skip links the wave-level walk follows, root in record 0.
void build_shadow_tree(const std::vector<hiprz_instance>& dinst, const std::vector<uint32_t>& members, std::vector<uint32_t>& rec,
                       std::vector<uint32_t>& order) {
    auto box_of = [&](uint32_t i) { return packed_instance_box(dinst[i]); };
    auto grow = [](InstanceBox& b, const InstanceBox& o) {
        for (int a = 0; a < 3; ++a) b.mn[a] = std::min(b.mn[a], o.mn[a]), b.mx[a] = std::max(b.mx[a], o.mx[a]);
    };
    auto area = [](const InstanceBox& b) {
        const float x = b.mx[0] - b.mn[0], y = b.mx[1] - b.mn[1], z = b.mx[2] - b.mn[2];
        return x * y + y * z + z * x;
    };
    const uint32_t n = uint32_t(members.size());
    order = members, rec.assign(size_t(2u * n) * 16u, RZ_END);
    std::vector<uint32_t> sorted, best;
    std::vector<float> left_area;
    struct Task {
        uint32_t node, lo, hi, link;
    };
    std::vector<Task> stack{{0u, 0u, n, RZ_END}};
    uint32_t next_free = 1u;
    while (!stack.empty()) {
        const Task t = stack.back();
        stack.pop_back();
        InstanceBox b = box_of(order[t.lo]);
        for (uint32_t k = t.lo + 1u; k < t.hi; ++k) grow(b, box_of(order[k]));
        const float interleaved[6] = {b.mn[0], b.mx[0], b.mn[1], b.mx[1], b.mn[2], b.mx[2]};
        uint32_t* r = &rec[size_t(t.node) * 16u];
        std::memcpy(r, interleaved, 24);
        for (int o = 0; o < 8; ++o) r[8 + o] = t.link;  // (only the wave-level walk follows this tree: the order of octant 0 under every octant)
        const uint32_t len = t.hi - t.lo;
        if (len == 1u) {
            r[6] = t.lo, r[7] = HIPRZ_NODE_LEAF | 1u;
            continue;
        }
        // the cheapest cut of the instances sorted by box centre along one of the axes: area(left) * |left| + area(right) * |right|
        float best_cost = 3.0e38f;
        uint32_t best_axis = 0u, best_cut = len / 2u;
        for (uint32_t axis = 0; axis < 3u; ++axis) {
            sorted.assign(order.begin() + t.lo, order.begin() + t.hi);
            std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) {
                const InstanceBox bx = box_of(x), by = box_of(y);
                return bx.mn[axis] + bx.mx[axis] < by.mn[axis] + by.mx[axis];
            });
            left_area.assign(len, 0.0f);
            InstanceBox acc = box_of(sorted[0]);
            for (uint32_t k = 1u; k < len; ++k) left_area[k] = area(acc), grow(acc, box_of(sorted[k]));  // area of the first k
            acc = box_of(sorted[len - 1u]);
            for (uint32_t k = len - 1u; k >= 1u; --k) {  // cut before position k
                const float cost = left_area[k] * float(k) + area(acc) * float(len - k);
                if (cost < best_cost) best_cost = cost, best_axis = axis, best_cut = k, best = sorted;
                grow(acc, box_of(sorted[k - 1u]));
            }
        }
        if (best.size() != len) best.assign(order.begin() + t.lo, order.begin() + t.hi);
        std::copy(best.begin(), best.end(), order.begin() + t.lo);
        best.clear();
        const uint32_t first = next_free;
        next_free += 2u;
        r[6] = first, r[7] = (2u - best_axis) << HIPRZ_NODE_PTYPE_SHIFT;  // the lower child along the axis first
        stack.push_back({first + 1u, t.lo + best_cut, t.hi, t.link});
        stack.push_back({first, t.lo, t.lo + best_cut, first + 1u});
    }
}

}  // namespace hiprz
