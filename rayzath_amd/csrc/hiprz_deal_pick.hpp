// hiprz_deal_pick.hpp — the integer half of dealing a leaf's later triangle pairs over a wave's lanes (dealt_visit, hiprz_device.hpp).
// A lane that holds a visit of a one-leaf mesh on its own tests pair 0 itself and has `rem` pairs left; the wave's left pairs, T in all,
// are work items 0 .. T - 1 in lane order of their owners, each owner's in pair order, and work item w goes to lane w % 64 in trip
// w / 64.  No floating-point arithmetic and no HIP header: tests/test_deal_pick.py compiles it with g++ under sanitizers beside a
// literal restatement of "every owner walks its pairs 1 .. in order".
#pragma once
#include <stdint.h>

#ifndef RZ_DEV  // (hiprz_device.hpp defines it for the device before it includes this file)
#define RZ_DEV inline
#endif

namespace hiprz {

constexpr uint32_t kDealLanes = 64u;
constexpr uint32_t kDealNoHit = 0xFFFFFFFFu;  // a result's distance word when the pair was missed; no lane when no helper hit
constexpr uint32_t kDealExternal = 0x80000000u;  // a result's triangle word: the facing bit rides on the index's top bit

// the trip and the lane a work item falls into, and the trips T work items take
RZ_DEV uint32_t deal_chunk(uint32_t work) { return work / kDealLanes; }
RZ_DEV uint32_t deal_lane(uint32_t work) { return work % kDealLanes; }
RZ_DEV uint32_t deal_chunks(uint32_t total) { return (total + kDealLanes - 1u) / kDealLanes; }

// The decline rule.  Left alone the wave takes max_rem further trips of the pair step; dealt it takes deal_chunks(total), and each of
// those costs about two plain trips: the owner search, a dozen pulls and the merge stand beside the step.  So dealing
// is taken when 2 * chunks + 1 <= max_rem — and only up to kDealMaxChunks trips: a helper's pulls overwrite the local ray it held as
// an owner, so a second trip would have to keep every owner's ray in registers of its own, which the five-wave build does not have.
constexpr uint32_t kDealMaxChunks = 1u;
constexpr uint32_t kDealMinRem = 2u * kDealMaxChunks + 1u;  // with one trip the rule is: total <= 64 and some owner has 3 pairs left
constexpr uint32_t kDealMaxOwners = kDealMaxChunks * kDealLanes / kDealMinRem;  // more owners with kDealMinRem left each would not fit
RZ_DEV bool deal_taken(uint32_t total, uint32_t max_rem) {
    const uint32_t chunks = deal_chunks(total);
    return total != 0u && chunks <= kDealMaxChunks && 2u * chunks + 1u <= max_rem;
}

// The owner of work item `work`: the lowest lane whose INCLUSIVE prefix of rem exceeds it (work < total, so there is one).  Six steps
// of a binary search; at(k) = the inclusive prefix held by lane k — on the device one ds_bpermute_b32, in the test an array read.
template <class At>
RZ_DEV uint32_t deal_owner(uint32_t work, const At& at) {
    uint32_t o = 0u;
    if (at(o + 31u) <= work) o += 32u;
    if (at(o + 15u) <= work) o += 16u;
    if (at(o + 7u) <= work) o += 8u;
    if (at(o + 3u) <= work) o += 4u;
    if (at(o + 1u) <= work) o += 2u;
    if (at(o) <= work) o += 1u;
    return o;
}
// the pair of its owner's leaf a work item stands for: the owner's own pair 0 is not dealt, its first left pair is 1
RZ_DEV uint32_t deal_pair(uint32_t work, uint32_t owner_exclusive) { return work - owner_exclusive + 1u; }

// The merge.  Every pair is tested against a range that contains the visit's final one, so the visit's hit is the nearest accepted
// distance and, among equal distances, the lowest triangle index.  Distances are positive floats: their bits order like they do.  An
// owner reads its helpers in pair order, which is triangle order, and keeps a result only when it is STRICTLY nearer than what it
// holds: that is the minimum on (distance, triangle index).  The owner's own pair 0 was tested first and gave the helpers their far
// end, so a helper's accepted distance is strictly below it and pair 0 needs no word in the merge.
RZ_DEV bool deal_nearer(uint32_t t_bits, uint32_t best_bits) { return t_bits < best_bits; }
// the same rule spelled on both words, for results met in any order (the test holds deal_nearer in pair order to it)
RZ_DEV bool deal_better(uint32_t t_bits, uint32_t triangle, uint32_t best_bits, uint32_t best_triangle) {
    return t_bits < best_bits || (t_bits == best_bits && t_bits != kDealNoHit && (triangle & ~kDealExternal) < (best_triangle & ~kDealExternal));
}

}  // namespace hiprz
