// hiprz_pair_pick.hpp — how the one-leaf walk settles two triangles that were tested in one iteration (tri_hit2 and tri_pair_step,
// hiprz_device.hpp).  Four compares and selects, no HIP header: tests/test_pair_pick.py compiles it with g++ under sanitizers beside
// the one-by-one loop it stands for.
#pragma once
#include <stdint.h>

#ifndef RZ_DEV  // (hiprz_device.hpp defines it for the device before it includes this file)
#define RZ_DEV inline
#endif

namespace hiprz {

struct PairPick {
    uint32_t winner;  // 0: neither triangle is accepted, 1: triangle a is the hit the iteration ends with, 2: triangle b
    float far_;       // the far end of the range after the iteration
};

// Triangles a and b stand one behind the other in leaf order.  inside_a / inside_b (bit 0 / bit 1 of `inside`): the triangle passed everything of tri_hit that
// does not look at the far end (barycentrics within the triangle, !(t <= near): the near end is the same for both, no hit moves it
// within a visit).  The one-by-one loop accepts a iff !(t_a >= far), which makes t_a the far end, and then b iff !(t_b >= that far end):
// b wins over a only when it is strictly nearer, so the first in leaf order wins among equal distances.  Written with the negated
// compare of tri_hit (`t >= far` rejects), so a NaN on either side decides as it does there.
RZ_DEV PairPick pair_pick(bool inside_a, bool inside_b, float t_a, float t_b, float far_) {
    const bool a = inside_a && !(t_a >= far_);
    const float far_a = a ? t_a : far_;
    const bool b = inside_b && !(t_b >= far_a);
    PairPick p;
    p.winner = b ? 2u : (a ? 1u : 0u);
    p.far_ = b ? t_b : far_a;
    return p;
}
RZ_DEV PairPick pair_pick(uint32_t inside, float t_a, float t_b, float far_) {
    return pair_pick((inside & 1u) != 0u, (inside & 2u) != 0u, t_a, t_b, far_);
}

}  // namespace hiprz
