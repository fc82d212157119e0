// view_delivery_check.cpp — RayZath::Hip::Engine::bakedView: the scene file argv[1] is loaded and rendered once (which uploads it and its
// camera), the argv[3] x argv[4] source records of argv[2] are viewed through the chart map of argv[5] (one uint32_t base per instance) and
// argv[6] (hiprz_gather_chart records) with the filter argv[12]: with the field of the probes argv[7], the grid argv[8], the records argv[9]
// and the visibility records argv[10] under bias argv[13] and max_back argv[14] — records to argv[11], the float image to argv[11] +
// ".image" — and without a field to argv[11] + ".plain", for tests/test_view_gpu.py to compare with Context.view.  A view before any world
// was rendered must be refused with HIPRZ_ERR_STATE, a source of another size, a filter the library does not know and a chart map for
// another number of instances must throw HIPRZ_ERR_INVALID.  Prints "VIEW DELIVERY OK".
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
    if (argc != 15) return std::printf("usage: view_delivery_check scene.json source.bin W H base.bin uv.bin probes.bin grid.bin sh.bin vis.bin out.bin filter bias max_back\n"), 2;
    try {
        std::vector<Engine::Record> source;
        Engine::ChartMap charts;
        std::vector<hiprz_bake_point> probes;
        std::vector<hiprz_field_grid> grids;
        std::vector<hiprz_probe_sh> sh;
        std::vector<hiprz_field_vis> vis;
        if (!read_all(argv[2], source) || !read_all(argv[5], charts.base) || !read_all(argv[6], charts.uv) || !read_all(argv[7], probes) || !read_all(argv[8], grids) ||
            !read_all(argv[9], sh) || !read_all(argv[10], vis) || grids.size() != 1)
            return std::printf("DIFFERENT: cannot open an input\n"), 1;
        const uint32_t W = uint32_t(std::atoi(argv[3])), H = uint32_t(std::atoi(argv[4])), filter = uint32_t(std::atoi(argv[12]));
        const hiprz_field_params params{float(std::atof(argv[13])), uint32_t(std::strtoul(argv[14], nullptr, 10)), {0u, 0u}};
        const hiprz_view_field field{&grids[0], probes.data(), sh.data(), vis.data(), probes.size(), &params};
        const float sky[3] = {0.25f, 0.5f, 2.0f};
        World world;
        IO::LoadLog log;
        IO::loadScene(argv[1], world, log);
        {
            Engine idle(0, 1);
            const int code = thrown([&] { idle.bakedView(source, W, H, charts, &field, sky, filter); });
            if (code != HIPRZ_ERR_STATE) return std::printf("DIFFERENT: a view before any world was rendered gave %d, not HIPRZ_ERR_STATE\n", code), 1;
        }
        RenderConfig cfg;
        cfg.tracing.max_depth = 2, cfg.tracing.rpp = 1;
        Engine engine(0, 1);
        engine.renderWorld(world, cfg);
        if (thrown([&] { engine.bakedView(source, W + 1u, H, charts, &field, sky, filter); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: a source of another size was taken\n"), 1;
        if (thrown([&] { engine.bakedView(source, W, H, charts, &field, sky, 2u); }) != HIPRZ_ERR_INVALID) return std::printf("DIFFERENT: filter 2 was taken\n"), 1;
        Engine::ChartMap other = charts;
        other.base.push_back(HIPRZ_GATHER_NONE);
        if (thrown([&] { engine.bakedView(source, W, H, other, &field, sky, filter); }) != HIPRZ_ERR_INVALID)
            return std::printf("DIFFERENT: a chart map for another number of instances was taken\n"), 1;
        std::vector<float> image;
        const std::vector<hiprz_view_pixel> pixels = engine.bakedView(source, W, H, charts, &field, sky, filter, &image);
        const std::vector<hiprz_view_pixel> again = engine.bakedView(source, W, H, charts, &field, sky, filter);
        if (pixels.empty() || pixels.size() != again.size() || std::memcmp(pixels.data(), again.data(), pixels.size() * sizeof(hiprz_view_pixel)) != 0)
            return std::printf("DIFFERENT: the same view twice differs\n"), 1;
        if (image.size() != 4u * pixels.size()) return std::printf("DIFFERENT: the image is not four floats per pixel\n"), 1;
        const std::vector<hiprz_view_pixel> plain = engine.bakedView(source, W, H, charts, nullptr, sky, filter);
        size_t kinds[5] = {0, 0, 0, 0, 0};
        for (size_t i = 0; i < pixels.size(); ++i) {
            const uint32_t kind = pixels[i].word >> HIPRZ_VIEW_KIND_SHIFT;
            if (kind > HIPRZ_VIEW_BACK) return std::printf("DIFFERENT: pixel %zu has kind %u\n", i, kind), 1;
            ++kinds[kind];
            if (std::memcmp(pixels[i].rgb, &image[4u * i], 12u) != 0 || image[4u * i + 3u] != 1.0f) return std::printf("DIFFERENT: the image differs from the records at pixel %zu\n", i), 1;
        }
        if (!write_all(argv[11], pixels) || !write_all(std::string(argv[11]) + ".image", image) || !write_all(std::string(argv[11]) + ".plain", plain))
            return std::printf("DIFFERENT: cannot write %s\n", argv[11]), 1;
        std::printf("%zu pixels: %zu none, %zu atlas, %zu field, %zu sky, %zu back\nVIEW DELIVERY OK\n", pixels.size(), kinds[0], kinds[1], kinds[2], kinds[3], kinds[4]);
        return 0;
    } catch (const Exception& e) {
        return std::printf("DIFFERENT: exception %d: %s\n", e.code, e.what()), 1;
    }
}
