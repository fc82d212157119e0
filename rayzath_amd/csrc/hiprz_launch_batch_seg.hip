// hiprz_launch_batch_seg.hip — the resident batch kernel in pass segments (rz_batch_seg_kernel): every tile's passes cut into S
// self-scheduled segments so that the launch ends on short units.  A translation unit of its own: its instantiations compile beside
// those of hiprz_launch_batch.hip.
#include <algorithm>

#include "hiprz_ctx.hpp"
#include "hiprz_kernels.hpp"

namespace hiprz {
namespace {

template <bool COUNT, int M, bool L, int SHADING, int WAVES>
void launch_seg(hiprz_ctx* c, const DFrame& f, uint32_t n, uint32_t segments, const BatchVariant& v) {
    constexpr auto kernel = &rz_batch_seg_kernel<COUNT, M, L, SHADING, WAVES>;
    const size_t lds = v.lds + 16u;  // + the item broadcast behind the park
    // the grid is what the chip holds at once (a workgroup takes items until the queue is empty), never more than there are items
    if (c->seg_occ_kernel != reinterpret_cast<const void*>(kernel) || c->seg_occ_lds != lds) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds) != hipSuccess) (void)hipGetLastError(), per_cu = 0;
        c->seg_occ_kernel = reinterpret_cast<const void*>(kernel), c->seg_occ_lds = lds, c->seg_occ_blocks = std::max(per_cu, 1);
    }
    const uint32_t items = v.units * segments;
    const dim3 grid(std::min(uint32_t(c->seg_occ_blocks) * c->n_cus, items));
    RZ_LAUNCH((rz_batch_seg_kernel<COUNT, M, L, SHADING, WAVES>), grid, dim3(256), lds, c->stream, c->dscene, c->dcamera, make_config(c), f, n,
              v.park_offset, segments, v.units, c->seg_ctl.ptr);
}

template <bool COUNT, int M, bool L>
void launch_seg_shading(hiprz_ctx* c, const DFrame& f, uint32_t n, uint32_t segments, const BatchVariant& v) {
    if (v.five) launch_seg<COUNT, M, L, RZ_SHADOW_PLAIN, 5>(c, f, n, segments, v);
    else if (v.shading == RZ_SHADOW_PLAIN) launch_seg<COUNT, M, L, RZ_SHADOW_PLAIN, RZ_MIN_WAVES>(c, f, n, segments, v);
    else if (v.shading == RZ_SHADOW_NONE) launch_seg<COUNT, M, L, RZ_SHADOW_NONE, RZ_MIN_WAVES>(c, f, n, segments, v);
    else launch_seg<COUNT, M, L, 1, RZ_MIN_WAVES>(c, f, n, segments, v);
}

template <bool COUNT>
void launch_seg_t(hiprz_ctx* c, const DFrame& f, uint32_t n, uint32_t segments, const BatchVariant& v) {
    if (v.mode == 4) launch_seg_shading<COUNT, 4, true>(c, f, n, segments, v);
    else if (v.mode == 2 && v.lds_scene) launch_seg_shading<COUNT, 2, true>(c, f, n, segments, v);
    else if (v.mode == 2) launch_seg_shading<COUNT, 2, false>(c, f, n, segments, v);
    else if (v.lds_scene) launch_seg_shading<COUNT, 1, true>(c, f, n, segments, v);
    else launch_seg_shading<COUNT, 1, false>(c, f, n, segments, v);
}

}  // namespace

void launch_batch_segmented(hiprz_ctx* c, const DFrame& f, uint32_t n_passes, uint32_t segments, bool counted) {
    counted ? launch_seg_t<true>(c, f, n_passes, segments, c->plan.batch) : launch_seg_t<false>(c, f, n_passes, segments, c->plan.batch);
}

}  // namespace hiprz
