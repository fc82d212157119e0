// atlas_delivery_check.cpp — RayZath::Hip::Engine::bakeAtlas: the scene file argv[1] is loaded and rendered once (which uploads it), the
// parts given as pairs (instance index, file of hiprz_atlas_tri records) from argv[9] on are rasterised into a W x H atlas, baked with the
// cosine table of (K, S) under the seed and dilated by `rings` rings, and texels, samples and ring map are written to argv[2] one after the
// other for tests/test_atlas_gpu.py to compare with Context.bake_atlas.  The same call again must give the same bytes, an atlas of width 0
// and an instance the world does not have must throw HIPRZ_ERR_INVALID, and a call before any world was rendered must be refused with
// HIPRZ_ERR_STATE.  Prints "ATLAS DELIVERY OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_engine.hpp"
#include "scene_io.hpp"

using namespace RayZath::Hip;

int main(int argc, char** argv) {
    if (argc < 11 || (argc - 9) % 2 != 0) return std::printf("usage: atlas_delivery_check scene.json out.bin W H K S seed rings (instance tris.bin)+\n"), 2;
    try {
        const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4])), K = uint32_t(std::atoi(argv[5])), S = uint32_t(std::atoi(argv[6]));
        const uint32_t seed = uint32_t(std::strtoul(argv[7], nullptr, 10)), rings = uint32_t(std::atoi(argv[8]));
        std::vector<Engine::AtlasPart> parts;
        for (int k = 9; k + 1 < argc; k += 2) {
            Engine::AtlasPart part;
            part.instance = uint32_t(std::atoi(argv[k]));
            std::FILE* f = std::fopen(argv[k + 1], "rb");
            if (!f) return std::printf("DIFFERENT: cannot open %s\n", argv[k + 1]), 1;
            hiprz_atlas_tri t;
            while (std::fread(&t, sizeof t, 1, f) == 1) part.charts.push_back(t);
            std::fclose(f);
            parts.push_back(part);
        }
        const float near_ = 1e-3f, far_ = 1e3f;
        {
            Engine idle(0, 1);
            try {
                idle.bakeAtlas(parts, W, H, K, S, seed, rings, near_, far_);
                return std::printf("DIFFERENT: an atlas was baked before any world was rendered\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: an atlas without a scene failed with %d, not HIPRZ_ERR_STATE\n", e.code), 1;
            }
        }
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        try {
            engine.bakeAtlas(parts, 0, H, K, S, seed, rings, near_, far_);
            return std::printf("DIFFERENT: an atlas of width 0 was taken\n"), 1;
        } catch (const Exception& e) {
            if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: width 0 failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
        }
        try {
            std::vector<Engine::AtlasPart> elsewhere = parts;
            elsewhere[0].instance = 1000;
            engine.bakeAtlas(elsewhere, W, H, K, S, seed, rings, near_, far_);
            return std::printf("DIFFERENT: instance 1000 was taken\n"), 1;
        } catch (const Exception& e) {
            if (e.code != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: instance 1000 failed with %d, not HIPRZ_ERR_INVALID\n", e.code), 1;
        }
        const Engine::BakedAtlas baked = engine.bakeAtlas(parts, W, H, K, S, seed, rings, near_, far_);
        const Engine::BakedAtlas small = engine.bakeAtlas(parts, 8, 8, K == 16 ? 32 : 16, S, seed, 0, near_, far_);
        const Engine::BakedAtlas again = engine.bakeAtlas(parts, W, H, K, S, seed, rings, near_, far_);
        const size_t texels = size_t(W) * H;
        if (baked.texels.size() != texels || baked.samples.size() != texels || baked.ring.size() != texels || small.texels.size() != 64 || baked.width != W || baked.height != H)
            return std::printf("DIFFERENT: %zu texels for a %u x %u atlas\n", baked.texels.size(), W, H), 1;
        if (std::memcmp(baked.texels.data(), again.texels.data(), texels * sizeof(hiprz_bake_texel)) != 0 ||
            std::memcmp(baked.samples.data(), again.samples.data(), texels * sizeof(hiprz_atlas_sample)) != 0 ||
            std::memcmp(baked.ring.data(), again.ring.data(), texels * sizeof(uint32_t)) != 0)
            return std::printf("DIFFERENT: the same atlas after another one differs\n"), 1;
        size_t covered = 0, filled = 0, empty = 0;
        for (size_t i = 0; i < texels; ++i) {
            if (baked.ring[i] == 0u) ++covered;
            else if (baked.ring[i] == HIPRZ_ATLAS_NONE) ++empty;
            else ++filled;
            if ((baked.ring[i] == 0u) != (baked.samples[i].triangle != HIPRZ_ATLAS_NONE)) return std::printf("DIFFERENT: ring map and samples disagree at texel %zu\n", i), 1;
        }
        std::FILE* f = std::fopen(argv[2], "wb");
        if (!f) return std::printf("DIFFERENT: cannot write %s\n", argv[2]), 1;
        std::fwrite(baked.texels.data(), sizeof(hiprz_bake_texel), texels, f);
        std::fwrite(baked.samples.data(), sizeof(hiprz_atlas_sample), texels, f);
        std::fwrite(baked.ring.data(), sizeof(uint32_t), texels, f);
        std::fclose(f);
        std::printf("%u x %u: %zu covered, %zu filled by %u rings, %zu empty\nATLAS DELIVERY OK\n", W, H, covered, filled, rings, empty);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
