// place_delivery_check.cpp — RayZath::Hip::Engine::placeProbes: the scene file argv[1] is loaded and rendered once (which uploads it), the
// hiprz_bake_point records of argv[2] are placed under the one hiprz_place_params of argv[3] with the sphere table of K = argv[5],
// S = argv[6] and the seed argv[7]; the moved probes go to argv[4] and the records to argv[4] + ".records", for tests/test_place_gpu.py to
// compare with Context.place_probes.  A placement before any world was rendered must be refused with HIPRZ_ERR_STATE, an empty batch
// must come back empty, a K the library does not take and params with a reach of 0 must throw HIPRZ_ERR_INVALID, the same placement twice
// and the one without records must give the same probes.  Prints "PLACE DELIVERY OK".
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
    if (argc != 8) return std::printf("usage: place_delivery_check scene.json probes.bin params.bin out.bin K S seed\n"), 2;
    try {
        std::vector<hiprz_bake_point> probes;
        std::vector<hiprz_place_params> all_params;
        if (!read_all(argv[2], probes) || !read_all(argv[3], all_params) || all_params.size() != 1) return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const hiprz_place_params params = all_params[0];
        const uint32_t K = uint32_t(std::atoi(argv[5])), S = uint32_t(std::atoi(argv[6])), seed = uint32_t(std::strtoul(argv[7], nullptr, 10));
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        {
            Engine idle(0, 1);
            const int code = thrown([&] { idle.placeProbes(probes, params, nullptr, K, S, seed); });
            if (code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a placement before any world was rendered gave %d, not HIPRZ_ERR_STATE\n", code), 1;
        }
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        std::vector<hiprz_place_record> records(3);
        if (!engine.placeProbes({}, params, &records, K, S, seed).empty() || !records.empty()) return std::printf("DIFFERENT: an empty batch came back with records\n"), 1;
        if (thrown([&] { engine.placeProbes(probes, params, nullptr, 32, S, seed); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 32 was taken\n"), 1;
        hiprz_place_params bad = params;
        bad.reach = 0.0f;
        if (thrown([&] { engine.placeProbes(probes, bad, nullptr, K, S, seed); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a reach of 0 was taken\n"), 1;
        const std::vector<hiprz_bake_point> moved = engine.placeProbes(probes, params, &records, K, S, seed);
        std::vector<hiprz_place_record> again_records;
        const std::vector<hiprz_bake_point> again = engine.placeProbes(probes, params, &again_records, K, S, seed), bare = engine.placeProbes(probes, params, nullptr, K, S, seed);
        const size_t bytes = probes.size() * sizeof(hiprz_bake_point);
        if (moved.size() != probes.size() || records.size() != probes.size() || std::memcmp(moved.data(), again.data(), bytes) != 0 || std::memcmp(moved.data(), bare.data(), bytes) != 0 ||
            std::memcmp(records.data(), again_records.data(), records.size() * sizeof(hiprz_place_record)) != 0)
            return std::printf("DIFFERENT: the same placement twice, or the one without records, differs\n"), 1;
        size_t invalid = 0, states[3] = {0, 0, 0}, stuck = 0, moves = 0;
        for (const hiprz_place_record& r : records) {
            if (r.word == HIPRZ_PLACE_INVALID) {
                ++invalid;
                continue;
            }
            const uint32_t state = r.word & HIPRZ_PLACE_STATE_MASK;
            if (state > HIPRZ_PLACE_INSIDE) return std::printf("DIFFERENT: a record with state %u\n", state), 1;
            ++states[state], stuck += (r.word & HIPRZ_PLACE_STUCK) != 0u, moves += r.word >> 16;
        }
        if (!write_all(argv[4], moved) || !write_all(std::string(argv[4]) + ".records", records)) return std::printf("DIFFERENT: cannot write %s\n", argv[4]), 1;
        std::printf("%zu probes, %zu invalid, %zu clear, %zu near, %zu inside, %zu stuck, %zu moves\nPLACE DELIVERY OK\n", probes.size(), invalid, states[0], states[1], states[2], stuck,
                    moves);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
