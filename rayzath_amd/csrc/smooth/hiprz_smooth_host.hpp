// hiprz_smooth_host.hpp — the pure-host half of lightmap smoothing (include/hiprz_smooth.h): what a call is refused for before a device
// is asked anything, the params check, which form of the kernel the build runs and the plan of an iteration's launch.  No HIP header:
// tests/test_smooth_abi.py compiles hiprz_smooth_host.cpp with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_smooth_params;

// Which form rz_smooth_kernel takes at step 1 and at the larger steps: 1 = staged (a 16 x 16 block of one sub-lattice, its 20 x 20 halo in
// LDS), 0 = direct (one thread per texel, taps from global memory).  The arithmetic and every output byte are the same.  Shipped is what
// was faster on the MI355X (DESIGN.md §6 "Lightmap smoothing"); make SMOOTH_DEFS="-DRZ_SMOOTH_STAGED_S1=.. -DRZ_SMOOTH_STAGED_SN=.."
// builds the others.
#ifndef RZ_SMOOTH_STAGED_S1
#define RZ_SMOOTH_STAGED_S1 1
#endif
#ifndef RZ_SMOOTH_STAGED_SN
#define RZ_SMOOTH_STAGED_SN 1
#endif

namespace hiprz {

constexpr uint32_t kSmoothBlock = 16;                      // a workgroup's block is kSmoothBlock x kSmoothBlock texels, 256 threads
constexpr uint32_t kSmoothHalo = kSmoothBlock + 4;         // and its halo of two taps on every side
constexpr uint32_t kSmoothPlanes = 10;                     // position, normal, RGB, flag

// nullptr when `p` is what a call takes, else what is wrong with it
const char* smooth_params_refusal(const hiprz_smooth_params* p);

// nullptr when a call may go on, else what is wrong with it, in the documented order: a null pointer (any_null), bad params, W or H out of
// range.  Every refusal is HIPRZ_ERR_INVALID.
const char* smooth_refusal(bool any_null, const hiprz_smooth_params* p, uint32_t W, uint32_t H);

constexpr bool smooth_staged(uint32_t step) { return step == 1u ? RZ_SMOOTH_STAGED_S1 != 0 : RZ_SMOOTH_STAGED_SN != 0; }

// the grid of iteration `step` over W x H texels, in workgroups of kSmoothBlock x kSmoothBlock threads.  Direct: the blocks that tile the
// atlas.  Staged: per residue (x0, y0) of the sub-lattice — min(step, W) x min(step, H) of them hold a texel — the blocks that tile the
// residue's ceil(W / step) x ceil(H / step) lattice points (a residue with fewer has blocks that find nothing to do).
struct SmoothGrid {
    uint32_t x, y;            // workgroups
    uint32_t per_x, per_y;    // staged: blocks per residue along each axis (direct: x and y themselves)
};
SmoothGrid smooth_grid(uint32_t W, uint32_t H, uint32_t step, bool staged);

// true when the byte ranges [a, a + bytes) and [b, b + bytes) share a byte
bool smooth_overlap(const void* a, const void* b, size_t bytes);

// the capacity (in texels) a scratch or staging of `have` texels takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t smooth_capacity(size_t have, size_t need);

}  // namespace hiprz
