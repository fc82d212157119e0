// field_delivery_check.cpp — RayZath::Hip::Engine::bakeVisibility and ::lookupField: the scene file argv[1] is loaded and rendered once
// (which uploads it), the hiprz_bake_point records of argv[2] — the probes of the grid argv[3] (one hiprz_field_grid) — get their
// visibility records with the sphere table of K = argv[7], S = argv[8], the seed argv[9] and the reach argv[10], written to argv[6]; the
// points of argv[5] are then looked up in the field of those probes, the hiprz_probe_sh records of argv[4] and the visibility records just
// baked, with bias argv[11] and max_back argv[12], to argv[6] + ".lookup", and without visibility records to argv[6] + ".plain", for
// tests/test_field_gpu.py to compare with Context.bake_visibility and Context.lookup_field.  A bake before any world was rendered must be
// refused with HIPRZ_ERR_STATE — a lookup needs no world —, an empty batch must come back empty, a K the library does not take, a reach
// of 0 and a grid for another number of probes must throw HIPRZ_ERR_INVALID.  Prints "FIELD DELIVERY OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_engine.hpp"
#include "scene_io.hpp"

using namespace RayZath::Hip;

namespace {
template <typename T>
bool read_all(const char* path, std::vector<T>& out) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    T record;
    while (std::fread(&record, sizeof record, 1, f) == 1) out.push_back(record);
    std::fclose(f);
    return true;
}
template <typename T>
bool write_all(const std::string& path, const std::vector<T>& records) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fwrite(records.data(), sizeof(T), records.size(), f);
    std::fclose(f);
    return true;
}
// what `call` throws: the code of the Exception, HIPRZ_OK when it returns
template <typename Call>
int thrown(Call call) {
    try {
        call();
    } catch (const Exception& e) {
        return e.code;
    }
    return HIPRZ_OK;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 13) return std::printf("usage: field_delivery_check scene.json probes.bin grid.bin sh.bin points.bin out.bin K S seed reach bias max_back\n"), 2;
    try {
        std::vector<hiprz_bake_point> probes, points;
        std::vector<hiprz_field_grid> grids;
        std::vector<hiprz_probe_sh> sh;
        if (!read_all(argv[2], probes) || !read_all(argv[3], grids) || !read_all(argv[4], sh) || !read_all(argv[5], points) || grids.size() != 1)
            return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const hiprz_field_grid grid = grids[0];
        const uint32_t K = uint32_t(std::atoi(argv[7])), S = uint32_t(std::atoi(argv[8])), seed = uint32_t(std::strtoul(argv[9], nullptr, 10));
        const float reach = float(std::atof(argv[10]));
        const hiprz_field_params params{float(std::atof(argv[11])), uint32_t(std::strtoul(argv[12], nullptr, 10)), {0u, 0u}};
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        std::vector<hiprz_field_result> before;
        {
            Engine idle(0, 1);
            const int code = thrown([&] { idle.bakeVisibility(probes, reach, K, S, seed); });
            if (code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a bake before any world was rendered gave %d, not HIPRZ_ERR_STATE\n", code), 1;
            before = idle.lookupField(grid, probes, sh, {}, points, params);  // no world: a lookup needs none
        }
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.bakeVisibility({}, reach, K, S, seed).empty() || !engine.lookupField(grid, probes, sh, {}, {}, params).empty())
            return std::printf("DIFFERENT: an empty batch came back with records\n"), 1;
        if (thrown([&] { engine.bakeVisibility(probes, reach, 32, S, seed); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 32 was taken\n"), 1;
        if (thrown([&] { engine.bakeVisibility(probes, 0.0f, K, S, seed); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a reach of 0 was taken\n"), 1;
        hiprz_field_grid other = grid;
        other.n[0] += 1u;
        if (thrown([&] { engine.lookupField(other, probes, sh, {}, points, params); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a grid for another number of probes was taken\n"), 1;
        const std::vector<hiprz_field_vis> vis = engine.bakeVisibility(probes, reach, K, S, seed);
        const std::vector<hiprz_field_vis> again = engine.bakeVisibility(probes, reach, K, S, seed);
        if (vis.size() != probes.size() || std::memcmp(vis.data(), again.data(), vis.size() * sizeof(hiprz_field_vis)) != 0)
            return std::printf("DIFFERENT: the same bake twice differs\n"), 1;
        const std::vector<hiprz_field_result> weighted = engine.lookupField(grid, probes, sh, vis, points, params);
        const std::vector<hiprz_field_result> plain = engine.lookupField(grid, probes, sh, {}, points, params);
        if (weighted.size() != points.size() || plain.size() != points.size() || std::memcmp(plain.data(), before.data(), plain.size() * sizeof(hiprz_field_result)) != 0)
            return std::printf("DIFFERENT: the plain lookup depends on a world\n"), 1;
        size_t invalid = 0, front = 0, back = 0, missed = 0, unread = 0;
        for (const hiprz_field_vis& v : vis) {
            if (v.words[3] == HIPRZ_FIELD_INVALID) ++invalid;
            else front += v.words[0], back += v.words[1], missed += v.words[2];
        }
        for (const hiprz_field_result& r : weighted) unread += r.word == HIPRZ_FIELD_INVALID;
        if (!write_all(argv[6], vis) || !write_all(std::string(argv[6]) + ".lookup", weighted) || !write_all(std::string(argv[6]) + ".plain", plain))
            return std::printf("DIFFERENT: cannot write %s\n", argv[6]), 1;
        std::printf("%zu probes, %zu invalid, %zu front hits, %zu back hits, %zu misses; %zu points, %zu without a value\nFIELD DELIVERY OK\n", probes.size(), invalid, front, back,
                    missed, points.size(), unread);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
