// order_delivery_check.cpp — RayZath::Hip::Engine::castRays and ::occluded with ordered = true: the scene file argv[1] is loaded and rendered
// once (which uploads it), the hiprz_ray records of argv[2] are cast in caller order and in sorted order (argv[4] = 1: normalised on the
// device) and must agree in every byte; the ordered hits, then the ordered occlusion words, are written to argv[3] for
// tests/test_order_gpu.py to compare with Context.trace / Context.occluded.  An empty batch must come back empty, and an ordered query
// before any world was rendered must be refused with HIPRZ_ERR_STATE.  Prints "ORDER DELIVERY OK".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hip_engine.hpp"
#include "scene_io.hpp"

using namespace RayZath::Hip;

int main(int argc, char** argv) {
    if (argc != 5) return std::printf("usage: order_delivery_check scene.json rays.bin out.bin normalize\n"), 2;
    try {
        std::vector<hiprz_ray> rays;
        {
            std::FILE* f = std::fopen(argv[2], "rb");
            if (!f) return std::printf("DIFFERENT: cannot open %s\n", argv[2]), 1;
            hiprz_ray r;
            while (std::fread(&r, sizeof r, 1, f) == 1) rays.push_back(r);
            std::fclose(f);
        }
        const bool normalize = std::string(argv[4]) == "1";
        {
            Engine idle(0, 1);
            try {
                idle.castRays(rays, normalize, true);
                return std::printf("DIFFERENT: an ordered castRays answered before any world was rendered\n"), 1;
            } catch (const Exception& e) {
                if (e.code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: ordered castRays without a scene failed with %d, not HIPRZ_ERR_STATE\n", e.code), 1;
            }
        }
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (!engine.castRays({}, normalize, true).empty() || !engine.occluded({}, normalize, true).empty())
            return std::printf("DIFFERENT: an empty batch came back with records\n"), 1;
        const std::vector<hiprz_hit> plain = engine.castRays(rays, normalize, false), hits = engine.castRays(rays, normalize, true);
        const std::vector<uint32_t> plain_shadow = engine.occluded(rays, normalize, false), shadow = engine.occluded(rays, normalize, true);
        if (hits.size() != rays.size() || shadow.size() != rays.size() || plain.size() != rays.size() || plain_shadow.size() != rays.size())
            return std::printf("DIFFERENT: %zu hits and %zu words for %zu rays\n", hits.size(), shadow.size(), rays.size()), 1;
        if (std::memcmp(plain.data(), hits.data(), hits.size() * sizeof(hiprz_hit)) != 0) return std::printf("DIFFERENT: castRays(ordered = true) != castRays(ordered = false)\n"), 1;
        if (std::memcmp(plain_shadow.data(), shadow.data(), shadow.size() * sizeof(uint32_t)) != 0)
            return std::printf("DIFFERENT: occluded(ordered = true) != occluded(ordered = false)\n"), 1;
        size_t found = 0;
        for (size_t i = 0; i < rays.size(); ++i) found += hits[i].flags & HIPRZ_HIT_FOUND;
        std::FILE* f = std::fopen(argv[3], "wb");
        if (!f) return std::printf("DIFFERENT: cannot write %s\n", argv[3]), 1;
        std::fwrite(hits.data(), sizeof(hiprz_hit), hits.size(), f);
        std::fwrite(shadow.data(), sizeof(uint32_t), shadow.size(), f);
        std::fclose(f);
        std::printf("%zu rays, %zu hit\nORDER DELIVERY OK\n", rays.size(), found);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
