// gather_delivery_check.cpp — RayZath::Hip::Engine::gather and Engine::bakeBounceAtlas: the scene file argv[1] is loaded and rendered once
// (which uploads it), the hiprz_bake_point records of argv[2] are gathered over the W x H source of argv[3] (16-byte records) with the chart
// map Engine::chartMap makes from the parts — pairs of an instance index and a file of hiprz_atlas_tri records from argv[13] on — the
// cosine table of K = argv[7], S = argv[8], the seed argv[9] and the sky (0.25, 0.5, 2), and the texels are written to argv[6] for
// tests/test_gather_gpu.py to compare with Context.gather.  Then Engine::bakeBounceAtlas bakes the parts at W x H with the albedo of
// argv[10], the emission of argv[11] and argv[12] bounces; direct, indirect and ring map go to argv[6] + ".direct", ".indirect" and ".ring".
// A gather before any world was rendered must be refused with HIPRZ_ERR_STATE, an empty batch must come back empty, a K the library does
// not take, a source of the wrong size, a chart map for another number of instances and a bounce bake without parts must throw
// HIPRZ_ERR_INVALID.  Prints "GATHER DELIVERY OK".
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
    if (argc < 15 || (argc - 13) % 2 != 0)
        return std::printf("usage: gather_delivery_check scene.json points.bin source.bin W H out.bin K S seed albedo.bin emission.bin bounces {instance charts.bin}\n"), 2;
    try {
        std::vector<hiprz_bake_point> points;
        std::vector<Engine::Record> source, albedo, emission;
        if (!read_all(argv[2], points) || !read_all(argv[3], source) || !read_all(argv[10], albedo) || !read_all(argv[11], emission))
            return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const uint32_t W = uint32_t(std::atoi(argv[4])), H = uint32_t(std::atoi(argv[5]));
        const uint32_t K = uint32_t(std::atoi(argv[7])), S = uint32_t(std::atoi(argv[8])), seed = uint32_t(std::strtoul(argv[9], nullptr, 10));
        const uint32_t bounces = uint32_t(std::atoi(argv[12]));
        std::vector<Engine::AtlasPart> parts;
        for (int i = 13; i + 1 < argc; i += 2) {
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
            const int code = thrown([&] { idle.gather(points, source, W, H, charts, K, S, seed, sky); });
            if (code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a gather before any world was rendered gave %d, not HIPRZ_ERR_STATE\n", code), 1;
        }
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.gather({}, source, W, H, charts, K, S, seed, sky).empty()) return std::printf("DIFFERENT: an empty batch came back with texels\n"), 1;
        if (thrown([&] { engine.gather(points, source, W, H, charts, 48, S, seed, sky); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 48 was taken\n"), 1;
        if (thrown([&] { engine.gather(points, source, W + 1, H, charts, K, S, seed, sky); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a source of the wrong size was taken\n"), 1;
        if (thrown([&] { engine.gather(points, source, W, H, Engine::chartMap({}, n_instances + 1), K, S, seed, sky); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a chart map for another number of instances was taken\n"), 1;
        if (thrown([&] { Engine::chartMap(parts, 1); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a part outside the world's instances was mapped\n"), 1;
        if (thrown([&] { engine.bakeBounceAtlas({}, n_instances, W, H, albedo, emission, bounces); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a bounce bake without parts was taken\n"), 1;
        const std::vector<hiprz_gather_texel> texels = engine.gather(points, source, W, H, charts, K, S, seed, sky);
        const std::vector<hiprz_gather_texel> other = engine.gather(points, source, W, H, charts, K == 16 ? 32 : 16, S, seed, sky);
        const std::vector<hiprz_gather_texel> again = engine.gather(points, source, W, H, charts, K, S, seed, sky);
        if (texels.size() != points.size() || other.size() != points.size() || again.size() != points.size())
            return std::printf("DIFFERENT: %zu texels for %zu points\n", texels.size(), points.size()), 1;
        if (std::memcmp(texels.data(), again.data(), texels.size() * sizeof(hiprz_gather_texel)) != 0) return std::printf("DIFFERENT: the same gather after another table differs\n"), 1;
        size_t invalid = 0, read = 0, missed = 0;
        for (const hiprz_gather_texel& t : texels) {
            if (t.counts == HIPRZ_GATHER_INVALID)
                ++invalid;
            else
                read += t.counts & 0xFFFFu, missed += t.counts >> 16;
        }
        if (!write_all(argv[6], texels)) return std::printf("DIFFERENT: cannot write %s\n", argv[6]), 1;
        const Engine::BouncedAtlas baked = engine.bakeBounceAtlas(parts, n_instances, W, H, albedo, emission, bounces, K, S, 16, 4, seed, 2, sky, 1.0e-3f, 1.0e3f);
        if (baked.width != W || baked.height != H || baked.direct.size() != size_t(W) * H || baked.indirect.size() != baked.direct.size() || baked.ring.size() != baked.direct.size())
            return std::printf("DIFFERENT: the atlas came back with %zu texels for %u x %u\n", baked.direct.size(), W, H), 1;
        const std::string out = argv[6];
        if (!write_all(out + ".direct", baked.direct) || !write_all(out + ".indirect", baked.indirect) || !write_all(out + ".ring", baked.ring))
            return std::printf("DIFFERENT: cannot write the atlas\n"), 1;
        std::printf("%zu points, %zu invalid, %zu rays read a texel, %zu missed; atlas %u x %u, %u bounces\nGATHER DELIVERY OK\n", points.size(), invalid, read, missed, W, H, bounces);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
