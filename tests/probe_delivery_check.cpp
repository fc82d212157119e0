// probe_delivery_check.cpp — RayZath::Hip::Engine::bakeProbes: the scene file argv[1] is loaded and rendered once (which uploads it), the
// hiprz_bake_point records of argv[2] are baked over the W x H source of argv[3] (16-byte records) with the chart map Engine::chartMap
// makes from the parts — pairs of an instance index and a file of hiprz_atlas_tri records from argv[12] on — the sphere table of
// K = argv[7], S = argv[8], the disk table of light_K = argv[9], light_S = argv[10], the seed argv[11] and the sky (0.25, 0.5, 2); the
// records go to argv[6] and, without the light term, to argv[6] + ".gathered", for tests/test_probe_gpu.py to compare with
// Context.bake_probes.  A bake before any world was rendered must be refused with HIPRZ_ERR_STATE, an empty batch must come back empty, a
// K the library does not take, a source of the wrong size and a chart map for another number of instances must throw HIPRZ_ERR_INVALID, and
// Engine::probeIrradiance must be hiprz_probe_irradiance.  Prints "PROBE DELIVERY OK".
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
    if (argc < 14 || (argc - 12) % 2 != 0)
        return std::printf("usage: probe_delivery_check scene.json probes.bin source.bin W H out.bin K S light_K light_S seed {instance charts.bin}\n"), 2;
    try {
        std::vector<hiprz_bake_point> probes;
        std::vector<Engine::Record> source;
        if (!read_all(argv[2], probes) || !read_all(argv[3], source)) return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const uint32_t W = uint32_t(std::atoi(argv[4])), H = uint32_t(std::atoi(argv[5]));
        const uint32_t K = uint32_t(std::atoi(argv[7])), S = uint32_t(std::atoi(argv[8])), LK = uint32_t(std::atoi(argv[9])), LS = uint32_t(std::atoi(argv[10]));
        const uint32_t seed = uint32_t(std::strtoul(argv[11], nullptr, 10));
        std::vector<Engine::AtlasPart> parts;
        for (int i = 12; i + 1 < argc; i += 2) {
            Engine::AtlasPart part;
            part.instance = uint32_t(std::atoi(argv[i]));
            if (!read_all(argv[i + 1], part.charts)) return std::printf("DIFFERENT: cannot open %s\n", argv[i + 1]), 1;
            parts.push_back(part);
        }
        const float sky[3] = {0.25f, 0.5f, 2.0f};
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        const uint32_t n_instances = uint32_t(world.instances.size());
        const Engine::ChartMap charts = Engine::chartMap(parts, n_instances);
        {
            Engine idle(0, 1);
            const int code = thrown([&] { idle.bakeProbes(probes, source, W, H, charts, K, S, LK, LS, seed, sky); });
            if (code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a bake before any world was rendered gave %d, not HIPRZ_ERR_STATE\n", code), 1;
        }
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.bakeProbes({}, source, W, H, charts, K, S, LK, LS, seed, sky).empty()) return std::printf("DIFFERENT: an empty batch came back with records\n"), 1;
        if (thrown([&] { engine.bakeProbes(probes, source, W, H, charts, 48, S, LK, LS, seed, sky); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 48 was taken\n"), 1;
        if (thrown([&] { engine.bakeProbes(probes, source, W, H, charts, K, S, 3, LS, seed, sky); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: light_K = 3 was taken\n"), 1;
        if (thrown([&] { engine.bakeProbes(probes, source, W + 1, H, charts, K, S, LK, LS, seed, sky); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a source of the wrong size was taken\n"), 1;
        if (thrown([&] { engine.bakeProbes(probes, source, W, H, Engine::chartMap({}, n_instances + 1), K, S, LK, LS, seed, sky); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a chart map for another number of instances was taken\n"), 1;
        const std::vector<hiprz_probe_sh> records = engine.bakeProbes(probes, source, W, H, charts, K, S, LK, LS, seed, sky);
        const std::vector<hiprz_probe_sh> gathered = engine.bakeProbes(probes, source, W, H, charts, K, S, LK, LS, seed, sky, nullptr, false);
        const std::vector<hiprz_probe_sh> again = engine.bakeProbes(probes, source, W, H, charts, K, S, LK, LS, seed, sky);
        if (records.size() != probes.size() || gathered.size() != probes.size() || again.size() != probes.size())
            return std::printf("DIFFERENT: %zu records for %zu probes\n", records.size(), probes.size()), 1;
        if (std::memcmp(records.data(), again.data(), records.size() * sizeof(hiprz_probe_sh)) != 0) return std::printf("DIFFERENT: the same bake twice differs\n"), 1;
        size_t invalid = 0, read = 0, missed = 0, shadowed = 0;
        const float up[3] = {0.0f, 1.0f, 0.0f};
        float brightest = 0.0f;
        for (const hiprz_probe_sh& r : records) {
            uint32_t counts, shade;
            std::memcpy(&counts, &r.sh[0][3], 4), std::memcpy(&shade, &r.sh[1][3], 4);
            const std::array<float, 3> e = Engine::probeIrradiance(r, up);
            float direct_call[3];
            hiprz_probe_irradiance(&r, up, direct_call);
            if (std::memcmp(e.data(), direct_call, sizeof direct_call) != 0) return std::printf("DIFFERENT: Engine::probeIrradiance is not hiprz_probe_irradiance\n"), 1;
            if (counts == HIPRZ_PROBE_INVALID) {
                ++invalid;
                if (e[0] != 0.0f || e[1] != 0.0f || e[2] != 0.0f) return std::printf("DIFFERENT: an invalid record has an irradiance\n"), 1;
            } else {
                read += counts & 0xFFFFu, missed += counts >> 16, shadowed += shade;
                if (e[0] > brightest) brightest = e[0];
            }
        }
        if (!write_all(argv[6], records) || !write_all(std::string(argv[6]) + ".gathered", gathered)) return std::printf("DIFFERENT: cannot write %s\n", argv[6]), 1;
        std::printf("%zu probes, %zu invalid, %zu rays read a texel, %zu missed, %zu shadow rays shadowed; the brightest red irradiance upwards %.4f\nPROBE DELIVERY OK\n",
                    probes.size(), invalid, read, missed, shadowed, double(brightest));
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
