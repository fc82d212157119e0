// bake_delivery_check.cpp — RayZath::Hip::Engine::bakeOcclusion: the scene file argv[1] is loaded and rendered once (which uploads it), the
// hiprz_bake_point records of argv[2] are baked with the cosine table of K = argv[4], S = argv[5] under the seed argv[6], and the texels
// are written to argv[3] for tests/test_bake_gpu.py to compare with Context.bake_occlusion.  A second bake with another table and back must
// give the same bytes, an empty batch must come back empty, a K the library does not take must throw HIPRZ_ERR_INVALID, and a bake before
// any world was rendered must be refused with HIPRZ_ERR_STATE.  Prints "BAKE DELIVERY OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_engine.hpp"
#include "scene_io.hpp"

using namespace RayZath::Hip;

int main(int argc, char** argv) {
    if (argc != 7) return std::printf("usage: bake_delivery_check scene.json points.bin out.bin K S seed\n"), 2;
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
                idle.bakeOcclusion(points, K, S, seed);
                return std::printf("DIFFERENT: a bake answered before any world was rendered\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a bake without a scene failed with %d, not HIPRZ_ERR_STATE\n", e.code), 1;
            }
        }
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.bakeOcclusion({}, K, S, seed).empty()) return std::printf("DIFFERENT: an empty batch came back with texels\n"), 1;
        try {
            engine.bakeOcclusion(points, 48, S, seed);
            return std::printf("DIFFERENT: K = 48 was taken\n"), 1;
        } catch (const Exception& e) {
            if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: K = 48 failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
        }
        const std::vector<hiprz_bake_texel> texels = engine.bakeOcclusion(points, K, S, seed);
        const std::vector<hiprz_bake_texel> other = engine.bakeOcclusion(points, K == 16 ? 32 : 16, S, seed);
        const std::vector<hiprz_bake_texel> again = engine.bakeOcclusion(points, K, S, seed);
        if (texels.size() != points.size() || other.size() != points.size() || again.size() != points.size())
            return std::printf("DIFFERENT: %zu texels for %zu points\n", texels.size(), points.size()), 1;
        if (std::memcmp(texels.data(), again.data(), texels.size() * sizeof(hiprz_bake_texel)) != 0)
            return std::printf("DIFFERENT: the same bake after another table differs\n"), 1;
        size_t invalid = 0, occluded = 0;
        for (const hiprz_bake_texel& t : texels) {
            if (t.occluded == HIPRZ_BAKE_INVALID)
                ++invalid;
            else
                occluded += t.occluded;
        }
        std::FILE* f = std::fopen(argv[3], "wb");
        if (!f) return std::printf("DIFFERENT: cannot write %s\n", argv[3]), 1;
        std::fwrite(texels.data(), sizeof(hiprz_bake_texel), texels.size(), f);
        std::fclose(f);
        std::printf("%zu points, %zu invalid, %zu of %zu rays occluded\nBAKE DELIVERY OK\n", points.size(), invalid, occluded, (points.size() - invalid) * K);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
