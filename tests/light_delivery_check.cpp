// light_delivery_check.cpp — RayZath::Hip::Engine::bakeLight: the scene file argv[1] is loaded and rendered once (which uploads it), the
// hiprz_bake_point records of argv[2] are light-baked with the disk table of K = argv[4], S = argv[5] under the seed argv[6], and the texels
// are written to argv[3] for tests/test_light_gpu.py to compare with Context.bake_light; argv[3] + ".spot0" gets the bake of the first spot
// light alone.  A second bake with another table and back must give the same bytes, an empty batch must come back empty, a K the library
// does not take and a range outside the lights must throw HIPRZ_ERR_INVALID, and a bake before any world was rendered must be refused with
// HIPRZ_ERR_STATE.  With three more arguments — charts.bin (hiprz_atlas_tri records, placed as instance 0), W, H — Engine::bakeLightAtlas bakes
// them with two rings and writes the texels to argv[3] + ".atlas" and the ring map to argv[3] + ".ring"; no parts must throw HIPRZ_ERR_INVALID.
// Prints "LIGHT DELIVERY OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_engine.hpp"
#include "scene_io.hpp"

using namespace RayZath::Hip;

namespace {
bool write_texels(const std::string& path, const std::vector<hiprz_light_texel>& texels) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fwrite(texels.data(), sizeof(hiprz_light_texel), texels.size(), f);
    std::fclose(f);
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 7 && argc != 10) return std::printf("usage: light_delivery_check scene.json points.bin out.bin K S seed [charts.bin W H]\n"), 2;
    try {
        std::vector<hiprz_bake_point> points;
        {
            std::FILE* f = std::fopen(argv[2], "rb");
            if (!f) return std::printf("DIFFERENT: cannot open %s\n", argv[2]), 1;
            hiprz_bake_point p;
            while (std::fread(&p, sizeof p, 1, f) == 1) points.push_back(p);
            std::fclose(f);
        }
        const uint32_t K = uint32_t(std::atoi(argv[4])), S = uint32_t(std::atoi(argv[5])), seed = uint32_t(std::strtoul(argv[6], nullptr, 10));
        {
            Engine idle(0, 1);
            try {
                idle.bakeLight(points, K, S, seed);
                return std::printf("DIFFERENT: a light bake answered before any world was rendered\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a light bake without a scene failed with %d, not HIPRZ_ERR_STATE\n", e.code), 1;
            }
        }
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.bakeLight({}, K, S, seed).empty()) return std::printf("DIFFERENT: an empty batch came back with texels\n"), 1;
        try {
            engine.bakeLight(points, 48, S, seed);
            return std::printf("DIFFERENT: K = 48 was taken\n"), 1;
        } catch (const Exception& e) {
            if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 48 failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
        }
        const hiprz_light_range outside = {0, 1000, 0, 0}, spot0 = {0, 1, 0, 0};
        try {
            engine.bakeLight(points, K, S, seed, &outside);
            return std::printf("DIFFERENT: a range of 1000 spot lights was taken\n"), 1;
        } catch (const Exception& e) {
            if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a range outside the lights failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
        }
        const std::vector<hiprz_light_texel> texels = engine.bakeLight(points, K, S, seed);
        const std::vector<hiprz_light_texel> other = engine.bakeLight(points, K == 16 ? 32 : 16, S, seed);
        const std::vector<hiprz_light_texel> again = engine.bakeLight(points, K, S, seed);
        const std::vector<hiprz_light_texel> alone = engine.bakeLight(points, K, S, seed, &spot0);
        if (texels.size() != points.size() || other.size() != points.size() || again.size() != points.size() || alone.size() != points.size())
            return std::printf("DIFFERENT: %zu texels for %zu points\n", texels.size(), points.size()), 1;
        if (std::memcmp(texels.data(), again.data(), texels.size() * sizeof(hiprz_light_texel)) != 0)
            return std::printf("DIFFERENT: the same bake after another table differs\n"), 1;
        size_t invalid = 0, shadowed = 0, lit = 0;
        for (const hiprz_light_texel& t : texels) {
            if (t.shadowed == HIPRZ_LIGHT_INVALID)
                ++invalid;
            else
                shadowed += t.shadowed, lit += t.light[0] > 0.0f || t.light[1] > 0.0f || t.light[2] > 0.0f;
        }
        if (!write_texels(argv[3], texels) || !write_texels(std::string(argv[3]) + ".spot0", alone)) return std::printf("DIFFERENT: cannot write %s\n", argv[3]), 1;
        if (argc == 10) {
            Engine::AtlasPart part;
            part.instance = 0;
            std::FILE* f = std::fopen(argv[7], "rb");
            if (!f) return std::printf("DIFFERENT: cannot open %s\n", argv[7]), 1;
            hiprz_atlas_tri tri;
            while (std::fread(&tri, sizeof tri, 1, f) == 1) part.charts.push_back(tri);
            std::fclose(f);
            const uint32_t W = uint32_t(std::atoi(argv[8])), H = uint32_t(std::atoi(argv[9]));
            try {
                engine.bakeLightAtlas({}, W, H, K, S, seed);
                return std::printf("DIFFERENT: an atlas without parts was taken\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: an atlas without parts failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
            }
            const Engine::LitAtlas lit = engine.bakeLightAtlas({part}, W, H, K, S, seed, 2, 1.0e-3f, 1.0e3f);
            if (lit.width != W || lit.height != H || lit.texels.size() != size_t(W) * H || lit.ring.size() != lit.texels.size() || lit.samples.size() != lit.texels.size())
                return std::printf("DIFFERENT: the atlas came back with %zu texels for %u x %u\n", lit.texels.size(), W, H), 1;
            std::FILE* g = std::fopen((std::string(argv[3]) + ".ring").c_str(), "wb");
            if (!g || !write_texels(std::string(argv[3]) + ".atlas", lit.texels)) return std::printf("DIFFERENT: cannot write the atlas\n"), 1;
            std::fwrite(lit.ring.data(), sizeof(uint32_t), lit.ring.size(), g);
            std::fclose(g);
            std::printf("atlas %u x %u from %zu triangles\n", W, H, part.charts.size());
        }
        std::printf("%zu points, %zu invalid, %zu lit, %zu rays shadowed\nLIGHT DELIVERY OK\n", points.size(), invalid, lit, shadowed);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
