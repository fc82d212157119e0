// hiprz_launch_shade.hip — split pipeline, second half of a pass: everything of traceRay after the closest hit
// (cpu_engine_kernel.cpp:118-177) in rz_shade_kernel, and — for scenes with lights that are not staged in LDS — the pass's
// shadow rays (anyIntersection, :398-481) in a lean kernel of their own, walked in their own sorted order.
#include "hiprz_ctx.hpp"
#include "hiprz_kernels.hpp"

#ifndef RZ_PACKET_MINW
#define RZ_PACKET_MINW 4  // waves per SIMD the wave-level shadow walk's register budget is cut for (it takes 90 VGPRs: 5 waves)
#endif

namespace hiprz {
namespace {

// The two orders a shaded pass needs.  The next pass's ray order is needed by the shadow kernel only when it has no order of its own
// (HIPRZ_SHADOW_SORT=0); otherwise it is sorted on the auxiliary stream beside the shadow rays' sort and walk, and the main stream
// picks it up after them (join_sort).  (The shadow rays' sort first and alone, the ray sort beside the walk only: measured on E in
// round 4 with the runs sort, 41.8 against 41.4 ms per step, and again beside the wave-level shadow walk, 35.05 against 34.5 — two memory-bound sorts share the chip better than a sort and the walk.)
void sort_after_shading(hiprz_ctx* c, const DFrame& f) {
    launch_sort(c, f.shadow_key != nullptr);
    if (f.shadow_key) launch_shadow_sort(c);
}

template <bool FIRST, bool COUNT>
void launch_shade_t(hiprz_ctx* c, const DFrame& f) {
    const ShadeVariant& v = c->plan.shade;
    const DConfig cfg = make_config(c);
    const dim3 grid(v.grid), block(v.block);
#define RZ_SHADE(L, S) RZ_LAUNCH((rz_shade_kernel<FIRST, COUNT, L, S>), grid, block, v.lds, c->stream, c->dscene, c->dcamera, cfg, f, v.top_n)
    switch (v.shadow) {
        case RZ_SHADOW_COMPAT_DEFER: RZ_SHADE(false, RZ_SHADOW_COMPAT_DEFER); break;
        case RZ_SHADOW_COMPAT: RZ_SHADE(false, RZ_SHADOW_COMPAT); break;
        case RZ_SHADOW_PLAIN:
            if (v.lds_scene) RZ_SHADE(true, RZ_SHADOW_PLAIN);
            else RZ_SHADE(false, RZ_SHADOW_PLAIN);
            break;
        case RZ_SHADOW_NONE:
            if (v.lds_scene) RZ_SHADE(true, RZ_SHADOW_NONE);
            else RZ_SHADE(false, RZ_SHADOW_NONE);
            break;
        case RZ_SHADOW_DEFER: RZ_SHADE(false, RZ_SHADOW_DEFER); break;
        case 1: RZ_SHADE(true, 1); break;
        default: RZ_SHADE(false, 3); break;
    }
#undef RZ_SHADE
    if (v.follow == SHADOWS_NONE) return;
    sort_after_shading(c, f);
    const dim3 sgrid(v.follow_grid), sblock(v.follow_block);
    switch (v.follow) {
        case SHADOWS_PACKET: RZ_LAUNCH((rz_shadow_packet_kernel<FIRST, COUNT, RZ_PACKET_MINW>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f); break;
        case SHADOWS_PACKET_COLOUR: RZ_LAUNCH((rz_shadow_packet_kernel<FIRST, COUNT, RZ_PACKET_MINW, true>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f); break;
        case SHADOWS_COOP3_COLOUR: RZ_LAUNCH((rz_shadow_coop_kernel<FIRST, COUNT, 3, true>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f); break;
        case SHADOWS_COOP4: RZ_LAUNCH((rz_shadow_coop_kernel<FIRST, COUNT, 4>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f); break;
        case SHADOWS_SKIP6: RZ_LAUNCH((rz_shadow_kernel<FIRST, COUNT, 6>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f, v.follow_top_n); break;
        default: RZ_LAUNCH((rz_shadow_kernel<FIRST, COUNT, 4>), sgrid, sblock, v.follow_lds, c->stream, c->dscene, c->dcamera, cfg, f, v.follow_top_n); break;
    }
    join_sort(c);
}

}  // namespace

void launch_shade(hiprz_ctx* c, const DFrame& f, bool first, bool counted) {
    if (first) counted ? launch_shade_t<true, true>(c, f) : launch_shade_t<true, false>(c, f);
    else counted ? launch_shade_t<false, true>(c, f) : launch_shade_t<false, false>(c, f);
}

}  // namespace hiprz

#ifdef RZ_PHASE_STATS  // diagnostic build (tools/phase_stats.py): wave-level executions / active lanes of the shadow rays' wave-level walk
extern "C" int hiprz_read_shadow_phase_stats(unsigned long long out[40]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(hiprz::rz_phase), sizeof(hiprz::rz_phase));
    unsigned long long zero[40] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(hiprz::rz_phase), zero, sizeof(hiprz::rz_phase));
    return 0;
}
#endif
