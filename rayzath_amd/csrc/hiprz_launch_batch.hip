// hiprz_launch_batch.hip — the fused pass kernel (one kernel per pass; the resident pipeline's renderFirstPass) and the
// resident batch kernel (ONE launch takes every owned tile through all the cumulative passes of a render call).
#include <algorithm>

#include "hiprz_ctx.hpp"
#include "hiprz_kernels.hpp"

namespace hiprz {
namespace {

template <bool FIRST, bool COUNT>
void launch_fused_t(hiprz_ctx* c, const DFrame& f) {
    const FusedVariant& v = c->plan.fused;
    const DConfig cfg = make_config(c);
    const dim3 grid(v.grid), block(v.block);
    if (v.family == FUSED_COMPAT) RZ_LAUNCH((rz_compat_pass_kernel<FIRST, COUNT>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
    else if (v.mode == 4u) RZ_LAUNCH((rz_pass_kernel<FIRST, COUNT, 4, true>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
    else if (v.mode == 2u && v.lds_scene) RZ_LAUNCH((rz_pass_kernel<FIRST, COUNT, 2, true>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
    else if (v.mode == 2u) RZ_LAUNCH((rz_pass_kernel<FIRST, COUNT, 2, false>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
    else if (v.lds_scene) RZ_LAUNCH((rz_pass_kernel<FIRST, COUNT, 1, true>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
    else RZ_LAUNCH((rz_pass_kernel<FIRST, COUNT, 1, false>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f);
}

template <bool COUNT>
void launch_batch_t(hiprz_ctx* c, const DFrame& f, uint32_t n) {
    const BatchVariant& v = c->plan.batch;
    const DConfig cfg = make_config(c);
    const dim3 grid(v.grid), block(v.block);
    if (v.family == BATCH_WAVE) {
        if (v.shading == RZ_SHADOW_PLAIN && v.one_leaf) RZ_LAUNCH((rz_wave_batch_kernel<COUNT, RZ_SHADOW_PLAIN, 4, true>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n);
        else if (v.shading == RZ_SHADOW_PLAIN) RZ_LAUNCH((rz_wave_batch_kernel<COUNT, RZ_SHADOW_PLAIN, 4>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n);
        else if (v.one_leaf) RZ_LAUNCH((rz_wave_batch_kernel<COUNT, RZ_SHADOW_NONE, 4, true>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n);
        else RZ_LAUNCH((rz_wave_batch_kernel<COUNT, RZ_SHADOW_NONE, 4>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n);
        return;
    }
    const uint32_t segments = std::min(n, v.segment_cap);
    if (segments > 1u) {
        launch_batch_segmented(c, f, n, segments, COUNT);
        return;
    }
#define RZ_BATCH(M, L)                                                                                                                     \
    do {                                                                                                                                   \
        if (v.five) RZ_LAUNCH((rz_batch_kernel<COUNT, M, L, RZ_SHADOW_PLAIN, 5>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n, v.park_offset); \
        else if (v.shading == RZ_SHADOW_PLAIN) RZ_LAUNCH((rz_batch_kernel<COUNT, M, L, RZ_SHADOW_PLAIN>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n, v.park_offset); \
        else if (v.shading == RZ_SHADOW_NONE) RZ_LAUNCH((rz_batch_kernel<COUNT, M, L, RZ_SHADOW_NONE>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n, v.park_offset); \
        else RZ_LAUNCH((rz_batch_kernel<COUNT, M, L, 1>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, n, v.park_offset);   \
    } while (0)
    if (v.mode == 4u) RZ_BATCH(4, true);  // a one-leaf world: instance boxes tested up front
    else if (v.mode == 2u && v.lds_scene) RZ_BATCH(2, true);
    else if (v.mode == 2u) RZ_BATCH(2, false);
    else if (v.lds_scene) RZ_BATCH(1, true);
    else RZ_BATCH(1, false);
#undef RZ_BATCH
}

}  // namespace

void launch_fused(hiprz_ctx* c, const DFrame& f, bool first, bool counted) {
    if (first) counted ? launch_fused_t<true, true>(c, f) : launch_fused_t<true, false>(c, f);
    else counted ? launch_fused_t<false, true>(c, f) : launch_fused_t<false, false>(c, f);
}

void launch_batch(hiprz_ctx* c, const DFrame& f, uint32_t n_passes, bool counted, hipEvent_t before, hipEvent_t after) {
    if (before) (void)hipEventRecord(before, c->stream);
    counted ? launch_batch_t<true>(c, f, n_passes) : launch_batch_t<false>(c, f, n_passes);
    if (after) (void)hipEventRecord(after, c->stream);
}

}  // namespace hiprz
