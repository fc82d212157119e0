// smooth_delivery_check.cpp — RayZath::Hip::Engine::smoothTexels and the smooth argument of bakeLightAtlas / bakeBounceAtlas: the
// hiprz_bake_point records of argv[2] and the 16-byte records of argv[3] (W = argv[4], H = argv[5]) are smoothed under the params
// iterations = argv[7], radius = argv[8], plane = argv[9], sigma_colour = argv[10] BEFORE any world is rendered (the library takes no
// device view) and written to argv[6]; then the scene file argv[1] is loaded and rendered once (which uploads it), and the atlas of the
// parts — pairs of an instance index and a file of hiprz_atlas_tri records from argv[17] on — is light-baked (light_K = argv[13],
// light_S = argv[14], seed = argv[15]) and bounce-baked (K = argv[11], S = argv[12], bounces = argv[16], albedo (0.7, 0.6, 0.5), no
// emission, sky (0.01, 0.02, 0.03)) with those params, to argv[6] + ".lit", ".lit_ring", ".direct", ".indirect" and ".ring", for
// tests/test_smooth_gpu.py to compare with Context's.  Params the library does not take and arrays of the wrong size must throw
// HIPRZ_ERR_INVALID; a null smooth argument must give the bytes of the call without it.  Prints "SMOOTH DELIVERY OK".
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
template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
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
    if (argc < 19 || (argc - 17) % 2 != 0)
        return std::printf("usage: smooth_delivery_check scene.json points.bin records.bin W H out iterations radius plane sigma_colour K S light_K light_S seed bounces "
                           "{instance charts.bin}\n"), 2;
    try {
        std::vector<hiprz_bake_point> points;
        std::vector<Engine::Record> records;
        if (!read_all(argv[2], points) || !read_all(argv[3], records)) return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const uint32_t W = uint32_t(std::atoi(argv[4])), H = uint32_t(std::atoi(argv[5]));
        const std::string out = argv[6];
        const hiprz_smooth_params params{uint32_t(std::atoi(argv[7])), float(std::atof(argv[8])), float(std::atof(argv[9])), float(std::atof(argv[10]))};
        const uint32_t K = uint32_t(std::atoi(argv[11])), S = uint32_t(std::atoi(argv[12])), LK = uint32_t(std::atoi(argv[13])), LS = uint32_t(std::atoi(argv[14]));
        const uint32_t seed = uint32_t(std::strtoul(argv[15], nullptr, 10)), bounces = uint32_t(std::atoi(argv[16]));
        std::vector<Engine::AtlasPart> parts;
        for (int i = 17; i + 1 < argc; i += 2) {
            Engine::AtlasPart part;
            part.instance = uint32_t(std::atoi(argv[i]));
            if (!read_all(argv[i + 1], part.charts)) return std::printf("DIFFERENT: cannot open %s\n", argv[i + 1]), 1;
            parts.push_back(part);
        }
        {
            Engine idle(0, 1);  // no world yet: smoothing needs none
            const std::vector<Engine::Record> smoothed = idle.smoothTexels(points, records, W, H, params);
            if (!same(smoothed, idle.smoothTexels(points, records, W, H, params))) return std::printf("DIFFERENT: the same smoothing twice differs\n"), 1;
            hiprz_smooth_params bad = params;
            bad.iterations = 9u;
            if (thrown([&] { idle.smoothTexels(points, records, W, H, bad); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: iterations = 9 was taken\n"), 1;
            bad = params, bad.plane = -1.0f;
            if (thrown([&] { idle.smoothTexels(points, records, W, H, bad); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: plane = -1 was taken\n"), 1;
            if (thrown([&] { idle.smoothTexels(points, records, W + 1, H, params); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: arrays of the wrong size were taken\n"), 1;
            size_t changed = 0;
            for (size_t i = 0; i < records.size(); ++i) {
                if (smoothed[i].word != records[i].word) return std::printf("DIFFERENT: texel %zu came back with another word\n", i), 1;
                changed += std::memcmp(&smoothed[i], &records[i], sizeof(Engine::Record)) != 0;
            }
            if (!write_all(out, smoothed)) return std::printf("DIFFERENT: cannot write %s\n", out.c_str()), 1;
            std::printf("%zu texels smoothed, %zu changed\n", records.size(), changed);
        }
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        const uint32_t n_instances = uint32_t(world.instances.size());
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        const uint32_t AW = 64, AH = 48, rings = 2;
        const float sky[3] = {0.01f, 0.02f, 0.03f};
        const std::vector<Engine::Record> albedo(size_t(AW) * AH, Engine::Record{{0.7f, 0.6f, 0.5f}, 0u});
        const Engine::LitAtlas plain = engine.bakeLightAtlas(parts, AW, AH, LK, LS, seed, rings);
        const Engine::LitAtlas plain_null = engine.bakeLightAtlas(parts, AW, AH, LK, LS, seed, rings, 1.0e-3f, 3.0e38f, nullptr, nullptr);
        const Engine::LitAtlas lit = engine.bakeLightAtlas(parts, AW, AH, LK, LS, seed, rings, 1.0e-3f, 3.0e38f, nullptr, &params);
        if (!same(plain.texels, plain_null.texels) || !same(plain.ring, plain_null.ring)) return std::printf("DIFFERENT: a null smooth argument changed bakeLightAtlas\n"), 1;
        if (same(plain.texels, lit.texels)) return std::printf("DIFFERENT: smoothing changed no byte of bakeLightAtlas\n"), 1;
        if (!same(plain.ring, lit.ring)) return std::printf("DIFFERENT: smoothing changed the ring map\n"), 1;
        const Engine::BouncedAtlas bounced = engine.bakeBounceAtlas(parts, n_instances, AW, AH, albedo, {}, bounces, K, S, LK, LS, seed, rings, sky, 1.0e-3f, 3.0e38f, &params);
        const Engine::BouncedAtlas unsmoothed = engine.bakeBounceAtlas(parts, n_instances, AW, AH, albedo, {}, bounces, K, S, LK, LS, seed, rings, sky);
        if (same(bounced.indirect, unsmoothed.indirect)) return std::printf("DIFFERENT: smoothing changed no byte of bakeBounceAtlas\n"), 1;
        if (!write_all(out + ".lit", lit.texels) || !write_all(out + ".lit_ring", lit.ring) || !write_all(out + ".direct", bounced.direct) ||
            !write_all(out + ".indirect", bounced.indirect) || !write_all(out + ".ring", bounced.ring) || !write_all(out + ".unsmoothed", unsmoothed.indirect))
            return std::printf("DIFFERENT: cannot write beside %s\n", out.c_str()), 1;
        std::printf("SMOOTH DELIVERY OK\n");
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
