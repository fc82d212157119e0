// tests/test_deal_pick.py compiles this with g++ under ASan and UBSan beside rayzath_amd/csrc/hiprz_deal_pick.hpp.  A wave of 64 lanes;
// lane l owns a visit of n_pairs[l] pairs (0: it holds none, or its mesh box was missed).  Pair p of a visit carries one candidate: hit or
// not, a distance (positive float bits, drawn from a few values so that equal distances are common) and a triangle index that grows
// with p.  Reference: every owner walks its pairs 0, 1, ... in order, a candidate is accepted when it is hit and strictly nearer than
// the far end, which it then becomes.  Dealt: every owner tests pair 0; the pairs left are work items found through deal_owner /
// deal_pair / deal_chunk / deal_lane, each tested against the owner's far end after pair 0 by whatever lane it falls to, and merged
// by the owner in pair order with deal_nearer — and once more in a shuffled order with deal_better.  Both must end with the reference's
// (distance, triangle), and every pair must have been assigned exactly once, whether or not deal_taken would take the wave.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "hiprz_deal_pick.hpp"

using namespace hiprz;

struct Candidate {
    bool hit;
    uint32_t t, triangle;
};
struct Result {
    uint32_t t, triangle;  // t == kDealNoHit: nothing accepted
};
static bool same(Result a, Result b) { return a.t == b.t && (a.t == kDealNoHit || a.triangle == b.triangle); }

static long checked = 0, ties_across_lanes = 0, taken = 0, declined = 0, straddled = 0;

static void fail(const char* what, uint32_t lane) {
    printf("FAILED: %s (lane %u)\n", what, lane);
    exit(1);
}

static void wave(const uint32_t (&n_pairs)[64], uint32_t far0, std::mt19937& rng) {
    std::vector<std::vector<Candidate>> pairs(64);
    uint32_t triangle = 0u;
    for (uint32_t l = 0; l < 64u; ++l)
        for (uint32_t p = 0; p < n_pairs[l]; ++p) {
            const bool external = (rng() & 1u) != 0u;
            pairs[l].push_back(Candidate{(rng() % 3u) != 0u, 0x3F000000u + (rng() % 6u) * 0x1000u, (triangle + uint32_t(rng() & 1u)) | (external ? kDealExternal : 0u)});
            triangle += 2u;
        }
    // reference: every owner walks its pairs in order
    Result want[64];
    for (uint32_t l = 0; l < 64u; ++l) {
        uint32_t far_ = far0;
        want[l] = Result{kDealNoHit, 0u};
        for (const Candidate& c : pairs[l])
            if (c.hit && c.t < far_) far_ = c.t, want[l] = Result{c.t, c.triangle};
    }
    // dealt: pair 0 by the owner, the rest as work items
    uint32_t rem[64], incl[64], excl[64], far_after0[64], total = 0u, max_rem = 0u;
    Result own[64];
    for (uint32_t l = 0; l < 64u; ++l) {
        far_after0[l] = far0, own[l] = Result{kDealNoHit, 0u};
        if (n_pairs[l] != 0u && pairs[l][0].hit && pairs[l][0].t < far0) far_after0[l] = pairs[l][0].t, own[l] = Result{pairs[l][0].t, pairs[l][0].triangle};
        rem[l] = n_pairs[l] != 0u ? n_pairs[l] - 1u : 0u;
        excl[l] = total, total += rem[l], incl[l] = total;
        max_rem = std::max(max_rem, rem[l]);
    }
    if (deal_chunks(total) != (total + 63u) / 64u) fail("deal_chunks", 0u);
    const bool take = deal_taken(total, max_rem);
    if (take && !(total != 0u && deal_chunks(total) <= kDealMaxChunks && 2u * deal_chunks(total) + 1u <= max_rem)) fail("deal_taken took a wave the rule declines", 0u);
    if (take && !(deal_chunks(total) < max_rem)) fail("deal_taken took a wave that saves no trip", 0u);
    (take ? taken : declined) += 1;
    std::vector<std::vector<uint32_t>> assigned(64);
    for (uint32_t l = 0; l < 64u; ++l) assigned[l].assign(n_pairs[l], 0u);
    std::vector<Result> result(total);
    std::vector<uint32_t> seat(deal_chunks(total) * 64u, 0u);
    for (uint32_t w = 0; w < total; ++w) {
        if (deal_chunk(w) * 64u + deal_lane(w) != w || deal_lane(w) >= 64u || deal_chunk(w) >= deal_chunks(total)) fail("deal_chunk / deal_lane", w);
        seat[deal_chunk(w) * 64u + deal_lane(w)] += 1u;
        const uint32_t owner = deal_owner(w, [&](uint32_t k) { return incl[k & 63u]; });
        if (owner >= 64u || !(excl[owner] <= w && w < incl[owner])) fail("deal_owner", w);
        const uint32_t p = deal_pair(w, excl[owner]);
        if (p < 1u || p >= n_pairs[owner]) fail("deal_pair", w);
        assigned[owner][p] += 1u;
        if (deal_chunk(excl[owner]) != deal_chunk(incl[owner] - 1u)) straddled += 1;
        const Candidate& c = pairs[owner][p];
        result[w] = c.hit && c.t < far_after0[owner] ? Result{c.t, c.triangle} : Result{kDealNoHit, 0u};
    }
    for (uint32_t s : seat)
        if (s > 1u) fail("two work items on one lane of one trip", 0u);
    for (uint32_t l = 0; l < 64u; ++l) {
        for (uint32_t p = 1; p < n_pairs[l]; ++p)
            if (assigned[l][p] != 1u) fail("a pair was not assigned exactly once", l);
        // the owner's merge, in pair order
        Result got = Result{kDealNoHit, 0u};
        for (uint32_t q = 0; q < rem[l]; ++q)
            if (deal_nearer(result[excl[l] + q].t, got.t)) got = result[excl[l] + q];
        if (got.t == kDealNoHit) got = own[l];
        else if (own[l].t != kDealNoHit && !(got.t < own[l].t)) fail("a helper's distance is not below the owner's own", l);
        if (!same(got, want[l])) fail("merge in pair order", l);
        // and in any order, on both words
        std::vector<uint32_t> order(rem[l]);
        for (uint32_t q = 0; q < rem[l]; ++q) order[q] = q;
        std::shuffle(order.begin(), order.end(), rng);
        Result any = Result{kDealNoHit, 0xFFFFFFFFu};
        for (uint32_t q : order)
            if (deal_better(result[excl[l] + q].t, result[excl[l] + q].triangle, any.t, any.triangle)) any = result[excl[l] + q];
        if (any.t == kDealNoHit) any = own[l];
        if (!same(any, want[l])) fail("merge in shuffled order", l);
        uint32_t at_nearest = 0u;
        for (uint32_t q = 0; q < rem[l]; ++q) at_nearest += result[excl[l] + q].t != kDealNoHit && result[excl[l] + q].t == got.t;
        if (at_nearest > 1u) ties_across_lanes += 1;
        checked += 1;
    }
}

int main(int argc, char** argv) {
    const long draws = argc > 1 ? atol(argv[1]) : 1000;
    std::mt19937 rng(20261u);
    // the rule at the figures that matter: a wave full of cube visits declines, a few cube visits deal, nothing left declines
    if (deal_taken(320u, 5u) || deal_taken(0u, 0u) || deal_taken(0u, 5u) || deal_taken(10u, 2u) || deal_taken(65u, 5u)) fail("deal_taken accepts", 0u);
    if (!deal_taken(50u, 5u) || !deal_taken(64u, 5u) || !deal_taken(3u, 3u) || !deal_taken(1u * 12u, 12u)) fail("deal_taken declines", 0u);
    // exhaustive small: every rem in 0..3 on four lanes placed at the wave's ends and at a row's seam
    const uint32_t spots[4] = {0u, 15u, 16u, 63u};
    for (uint32_t code = 0; code < 256u; ++code) {
        uint32_t n[64] = {};
        for (uint32_t k = 0; k < 4u; ++k) n[spots[k]] = (code >> (2u * k)) & 3u ? ((code >> (2u * k)) & 3u) + 1u : 0u;
        for (int rep = 0; rep < 8; ++rep) wave(n, 0x7F000000u, rng);
    }
    // chosen totals: T = 0, 1, 63, 64, 65, 128, 320 — uniform (cubes: 6 pairs) and non-uniform
    const uint32_t totals[7] = {0u, 1u, 63u, 64u, 65u, 128u, 320u};
    for (uint32_t total : totals)
        for (int rep = 0; rep < 200; ++rep) {
            uint32_t n[64] = {}, left = total;
            if (total == 320u && rep % 2 == 0) {
                for (uint32_t l = 0; l < 64u; ++l) n[l] = 6u;
                left = 0u;
            }
            while (left != 0u) {
                const uint32_t l = rng() % 64u, take = 1u + rng() % std::min(left, 12u);
                if (n[l] == 0u) n[l] = 1u;
                n[l] += take, left -= take;
            }
            uint32_t sum = 0u;
            for (uint32_t l = 0; l < 64u; ++l) sum += n[l] ? n[l] - 1u : 0u;
            if (sum != total) fail("the test's own totals", total);
            wave(n, rep % 3 ? 0x7F000000u : 0x3F003000u, rng);
        }
    // random: a few owners of mixed leaves among quads (1 pair) and idle lanes
    for (long d = 0; d < draws; ++d) {
        uint32_t n[64];
        const uint32_t density = 1u + rng() % 8u;
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t kind = rng() % 8u;
            n[l] = kind >= density ? (rng() & 1u) : kind == 0u ? 1u + rng() % 16u : kind == 1u ? 6u : 1u + rng() % 3u;
        }
        wave(n, d % 4 ? 0x7F000000u : 0x3F002000u, rng);
    }
    if (ties_across_lanes == 0 || taken == 0 || declined == 0 || straddled == 0) fail("the draws did not reach a tie across lanes, a taken wave, a declined wave and a straddled owner", 0u);
    printf("%ld\n", checked);
    return 0;
}
