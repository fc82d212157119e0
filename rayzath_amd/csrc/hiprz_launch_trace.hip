// hiprz_launch_trace.hip — split pipeline, first half of a pass: the closest-hit walk of every owned pixel's ray
// (traverseWorld + closestIntersection, cpu_engine_kernel.cpp:254-352) -> a 20-byte hit record per pixel.
// Instantiates rz_trace_coop_kernel / rz_trace_skip_kernel / rz_trace_kernel (hiprz_kernels.hpp).
#include "hiprz_ctx.hpp"
#include "hiprz_kernels.hpp"

namespace hiprz {
namespace {

template <bool FIRST, bool COUNT>
void launch_trace_t(hiprz_ctx* c, const DFrame& f) {
    const TraceVariant& t = c->plan.trace;
    const dim3 grid(t.grid), block(t.block);
    if (t.family == TRACE_COMPAT) {
        RZ_LAUNCH((rz_trace_coop_compat_kernel<FIRST, COUNT>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, make_config(c), f);
    } else if (t.family == TRACE_COOP) {
        if (t.waves == 5u && t.one_leaf) RZ_LAUNCH((rz_trace_coop_kernel<FIRST, COUNT, 5, true>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else if (t.waves == 5u) RZ_LAUNCH((rz_trace_coop_kernel<FIRST, COUNT, 5>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else if (t.waves == 6u) RZ_LAUNCH((rz_trace_coop_kernel<FIRST, COUNT, 6>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else if (t.one_leaf) RZ_LAUNCH((rz_trace_coop_kernel<FIRST, COUNT, 4, true>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else RZ_LAUNCH((rz_trace_coop_kernel<FIRST, COUNT, 4>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
    } else if (t.family == TRACE_SKIP) {
        if (t.waves == 6u) RZ_LAUNCH((rz_trace_skip_kernel<FIRST, COUNT, 6>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f, t.top_n);
        else RZ_LAUNCH((rz_trace_skip_kernel<FIRST, COUNT, 4>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f, t.top_n);
    } else if (t.mode == 4u) {
        RZ_LAUNCH((rz_trace_kernel<FIRST, COUNT, 4, true>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
    } else if (t.mode == 2u) {
        if (t.lds_scene) RZ_LAUNCH((rz_trace_kernel<FIRST, COUNT, 2, true>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else RZ_LAUNCH((rz_trace_kernel<FIRST, COUNT, 2, false>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
    } else {
        if (t.lds_scene) RZ_LAUNCH((rz_trace_kernel<FIRST, COUNT, 1, true>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
        else RZ_LAUNCH((rz_trace_kernel<FIRST, COUNT, 1, false>), grid, block, t.lds, c->stream, c->dscene, c->dcamera, f);
    }
}

}  // namespace

void launch_trace(hiprz_ctx* c, const DFrame& f, bool first, bool counted) {
    if (first) counted ? launch_trace_t<true, true>(c, f) : launch_trace_t<true, false>(c, f);
    else counted ? launch_trace_t<false, true>(c, f) : launch_trace_t<false, false>(c, f);
}

}  // namespace hiprz

#ifdef RZ_PHASE_STATS  // diagnostic build (tools/phase_stats.py): wave-level executions / active lanes of the walk's step kinds
extern "C" int hiprz_read_phase_stats(unsigned long long out[40]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(hiprz::rz_phase), sizeof(hiprz::rz_phase));
    unsigned long long zero[40] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(hiprz::rz_phase), zero, sizeof(hiprz::rz_phase));
    return 0;
}
#endif
