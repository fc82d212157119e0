// hiprz_flat_pick.hpp — the integer half of the one-leaf-world walk (closest_hit_flat, hiprz_device.hpp): which instance a ray visits
// next, and where a round's visits go in the dense item list.  No floating-point arithmetic beyond eight compares and no HIP header:
// tests/test_flat_pick.py compiles it with g++ under sanitizers beside a literal restatement of the loops it replaced.
#pragma once
#include <stdint.h>

#ifndef RZ_DEV  // (hiprz_device.hpp defines it for the device before it includes this file)
#define RZ_DEV inline
#endif

namespace hiprz {

constexpr uint32_t kFlatNone = 0xFFFFFFFFu;  // = RZ_BIN_NONE: the ray has no candidate this round

RZ_DEV uint32_t flat_ctz(uint32_t v) { return uint32_t(__builtin_ctz(v)); }            // v != 0
RZ_DEV uint32_t flat_top_bit(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }  // v != 0

// the leaf's (at most 8) instance ids, 4 bits each: slot k of the leaf in bits 4k..4k+3
RZ_DEV uint32_t flat_pack_id(uint32_t packed, uint32_t k, uint32_t id) { return packed | ((id & 15u) << (4u * k)); }
RZ_DEV uint32_t flat_id(uint32_t packed, uint32_t k) { return (packed >> (4u * k)) & 15u; }
// bits of the slots a leaf of `count` instances has (count <= 8)
RZ_DEV uint32_t flat_slots(uint32_t count) { return (1u << count) - 1u; }
// bits of the slots k >= next (next <= 8)
RZ_DEV uint32_t flat_from(uint32_t next) { return ~((1u << next) - 1u); }

// bit k: slot k's box starts no farther than the range ends, !(tm[k] > far) — true for a NaN on either side, as in the one-by-one walk
RZ_DEV uint32_t flat_le_mask(const float (&tm)[8], float far_) {
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) m |= uint32_t(!(tm[k] > far_)) << k;
    return m;
}

// The next candidate of a ray: the first slot k >= next whose up-front verdict (bit k of mask) holds and whose box starts within the
// range as it is now.  The slots passed over are done with (a range only shrinks): next = k + 1.  Without a candidate the ray is
// finished: mask = 0, and next stands behind the last slot that was looked at.  Eight independent compares, then integer operations:
// what the chain "for k: if (no candidate yet && k >= next && bit k) { next = k + 1; if (!(tm[k] > far)) candidate = id k }" gives.
RZ_DEV uint32_t flat_pick(uint32_t ids, const float (&tm)[8], float far_, uint32_t& mask, uint32_t& next) {
    const uint32_t rest = mask & flat_from(next);
    const uint32_t alive = rest & flat_le_mask(tm, far_);
    if (alive != 0u) {
        const uint32_t k = flat_ctz(alive);
        next = k + 1u;
        return flat_id(ids, k);
    }
    if (rest != 0u) next = flat_top_bit(rest) + 1u;
    mask = 0u;
    return kFlatNone;
}

// flat_pick for the visit a ray makes in place, ahead of the binned rounds: bit i of `small` = instance i's mesh is one leaf of at most
// 4 triangles.  The candidate is flat_pick's; it is returned, and mask / next committed, only where its bit in `small` is set.
// Otherwise kFlatNone comes back with mask and next as they were, and the first binned round picks the same candidate again.  A ray
// without any candidate is finished as flat_pick finishes it.
RZ_DEV uint32_t flat_pick_first(uint32_t ids, const float (&tm)[8], float far_, uint32_t& mask, uint32_t& next, uint32_t small) {
    const uint32_t rest = mask & flat_from(next);
    const uint32_t alive = rest & flat_le_mask(tm, far_);
    if (alive != 0u) {
        const uint32_t k = flat_ctz(alive), id = flat_id(ids, k);
        if (((small >> id) & 1u) == 0u) return kFlatNone;
        next = k + 1u;
        return id;
    }
    if (rest != 0u) next = flat_top_bit(rest) + 1u;
    mask = 0u;
    return kFlatNone;
}

// ---- one scan for three prefix sums over the (at most 8) bins of a round ----
// bin k holds c = the lanes its visits want: 8 per visit of a wide instance, 1 otherwise.  Packed: bits 0-11 lanes of the wide bins
// (<= 256 visits x 8), 12-20 lanes of the other bins (<= 256), 21-29 visits of all bins (<= 256): no field carries into the next.
RZ_DEV uint32_t flat_pack_bin(uint32_t c, bool wide) { return wide ? (c | ((c >> 3) << 21)) : ((c << 12) | (c << 21)); }

template <int N>
struct FlatShift {};
// Inclusive prefix over lanes 0..7 in three steps.  shr(v, FlatShift<N>) = v of the lane N below, 0 where there is none — on the device a
// DPP row shift of one register (V = uint32_t), in the test all 8 lanes at once (V = an array).
template <class V, class Shr>
RZ_DEV V flat_prefix8(V incl, const Shr& shr) {
    incl += shr(incl, FlatShift<1>{});
    incl += shr(incl, FlatShift<2>{});
    incl += shr(incl, FlatShift<4>{});
    return incl;
}

struct FlatRound {  // a round's totals (lane 7 of the inclusive prefix): the same in every lane of every wave
    uint32_t n_visits, wide_lanes, narrow_lanes, n_items;
    bool split;  // wide visits get 8 lanes each, wide bins first; else (the lanes would not fit the workgroup, or no wide visit) one lane per visit
};
RZ_DEV FlatRound flat_round(uint32_t totals) {
    FlatRound r;
    r.n_visits = totals >> 21;
    r.wide_lanes = totals & 0xFFFu, r.narrow_lanes = (totals >> 12) & 0x1FFu;
    r.split = r.wide_lanes != 0u && r.wide_lanes + r.narrow_lanes <= 256u;
    r.n_items = r.split ? r.wide_lanes + r.narrow_lanes : r.n_visits;
    return r;
}
// first item slot of a visit: `before` = the exclusive packed prefix at the visit's bin, `rank` = what the bin's counter held before it
RZ_DEV uint32_t flat_item_slot(const FlatRound& r, uint32_t before, uint32_t rank, bool wide_item) {
    if (r.split && wide_item) return (before & 0xFFFu) + rank;
    if (r.split) return r.wide_lanes + ((before >> 12) & 0x1FFu) + rank;
    return (before >> 21) + (wide_item ? rank >> 3 : rank);
}

}  // namespace hiprz
