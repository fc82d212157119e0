// tests/test_flat_pick.py: rayzath_amd/csrc/hiprz_flat_pick.hpp against literal restatements of what it replaced, in a program of its
// own (g++ with ASan and UBSan).  Prints one line of counts; any difference ends it with a message and exit status 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "hiprz_flat_pick.hpp"

using namespace hiprz;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return uint32_t((z ^ (z >> 31)) >> 16);
}
static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// ---- the pick ----
// the walk's candidate search as it stood before flat_pick (closest_hit_binned, FLAT): order[] = the leaf's tlas_order entries
static uint32_t parent_pick(const uint32_t (&order)[8], const float (&tm)[8], float far_, uint32_t& flat_mask, uint32_t& flat_next) {
    uint32_t cand = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < 8u; ++k) {
        if (cand == 0xFFFFFFFFu && k >= flat_next && ((flat_mask >> k) & 1u)) {
            flat_next = k + 1u;
            if (!(tm[k] > far_)) cand = order[k];
        }
    }
    if (cand == 0xFFFFFFFFu) flat_mask = 0u;
    return cand;
}

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNan = std::numeric_limits<float>::quiet_NaN();
static const float kPool[] = {0.0f, -0.0f, kInf, -kInf, kNan, 1.0f, 1.0f, 2.0f, -1.0f, 0.5f, 3.402823466e+38f, 1.401298464e-45f, 1.00000012f};
// CLASS 0: every value from the pool (equal values, tm[k] == far, zeros of both signs, infinities, NaN); 1: far from the pool or one of
// the tm, tm random finite (tm[k] == far without specials); 2: everything random bit patterns (any float, NaNs of every payload)
static float draw(int cls) {
    if (cls == 0) return kPool[rnd() % (sizeof kPool / sizeof kPool[0])];
    if (cls == 1) return float(int(rnd() % 17u) - 8) * 0.25f;
    const uint32_t u = rnd() << 16 ^ rnd();
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static long check_picks(int draws) {
    long n = 0, with_candidate = 0, culled = 0, nan_seen = 0, equal_far = 0;
    for (uint32_t mask = 0; mask < 256u; ++mask) {
        for (uint32_t next = 0; next <= 8u; ++next) {
            for (int cls = 0; cls < 3; ++cls) {
                for (int d = 0; d < draws; ++d) {
                    float tm[8];
                    for (float& t : tm) t = draw(cls);
                    float far_ = draw(cls);
                    if (cls == 1 && (rnd() & 1u)) far_ = tm[rnd() & 7u];
                    uint32_t order[8], ids = 0u;
                    for (uint32_t k = 0; k < 8u; ++k) order[k] = (k * 5u + (rnd() & 15u)) & 15u, ids = flat_pack_id(ids, k, order[k]);
                    uint32_t m0 = mask, n0 = next, m1 = mask, n1 = next;
                    const uint32_t want = parent_pick(order, tm, far_, m0, n0);
                    const uint32_t got = flat_pick(ids, tm, far_, m1, n1);
                    if (want != got || m0 != m1 || n0 != n1) {
                        printf("pick differs: mask %02x next %u far %08x tm", mask, next, bits(far_));
                        for (float t : tm) printf(" %08x", bits(t));
                        printf(": candidate %u / %u, mask %02x / %02x, next %u / %u (parent / new)\n", want, got, m0, m1, n0, n1);
                        return -1;
                    }
                    n += 1, with_candidate += want != 0xFFFFFFFFu;
                    culled += want != 0xFFFFFFFFu && n0 > next + 1u;
                    for (float t : tm) nan_seen += t != t, equal_far += t == far_;
                }
            }
        }
    }
    // the draws reached what they are for
    if (with_candidate == 0 || culled == 0 || nan_seen == 0 || equal_far == 0) {
        printf("pick draws: %ld candidates, %ld behind a culled slot, %ld NaN, %ld tm == far\n", with_candidate, culled, nan_seen, equal_far);
        return -1;
    }
    return n;
}

// ---- the packed prefix ----
struct Row {  // the 16 lanes of a DPP row at once
    uint32_t v[16];
    Row& operator+=(const Row& o) {
        for (int i = 0; i < 16; ++i) v[i] += o.v[i];
        return *this;
    }
};
struct RowShr {  // row_shr:N with bound_ctrl: lane i takes lane i - N, lanes below N take 0
    template <int N>
    Row operator()(const Row& r, FlatShift<N>) const {
        Row o;
        for (int i = 0; i < 16; ++i) o.v[i] = i >= N ? r.v[i - N] : 0u;
        return o;
    }
};

// one round: visits[k] of bin k, `wide` = bit k: bin k's visits take 8 lanes.  Returns false on any difference.
static bool check_round(const uint32_t (&visits)[8], uint32_t wide) {
    Row own;
    uint32_t c[8];
    for (int i = 0; i < 16; ++i) own.v[i] = 0u;
    for (uint32_t k = 0; k < 8u; ++k) {
        const bool w = (wide >> k) & 1u;
        c[k] = w ? visits[k] * 8u : visits[k];
        own.v[k] = flat_pack_bin(c[k], w);
    }
    const Row incl = flat_prefix8(own, RowShr{});
    // three plain prefix sums
    uint32_t wide_lanes = 0u, narrow_lanes = 0u, n_visits = 0u;
    uint32_t wide_before[8], narrow_before[8], visits_before[8];
    for (uint32_t k = 0; k < 8u; ++k) {
        wide_before[k] = wide_lanes, narrow_before[k] = narrow_lanes, visits_before[k] = n_visits;
        if ((wide >> k) & 1u) wide_lanes += c[k];
        else narrow_lanes += c[k];
        n_visits += visits[k];
        const uint32_t p = incl.v[k];
        if ((p & 0xFFFu) != wide_lanes || ((p >> 12) & 0x1FFu) != narrow_lanes || (p >> 21) != n_visits) {
            printf("prefix differs at bin %u: packed %08x, plain %u %u %u\n", k, p, wide_lanes, narrow_lanes, n_visits);
            return false;
        }
    }
    const FlatRound r = flat_round(incl.v[7]);
    const bool split = wide_lanes != 0u && wide_lanes + narrow_lanes <= 256u;
    const uint32_t n_items = split ? wide_lanes + narrow_lanes : n_visits;
    if (r.n_visits != n_visits || r.wide_lanes != wide_lanes || r.narrow_lanes != narrow_lanes || r.split != split || r.n_items != n_items) {
        printf("totals differ: %u %u %u %d %u, plain %u %u %u %d %u\n", r.n_visits, r.wide_lanes, r.narrow_lanes, int(r.split), r.n_items, n_visits,
               wide_lanes, narrow_lanes, int(split), n_items);
        return false;
    }
    // every visit's slots: where the scatter as it stood put them, and together exactly [0, n_items)
    unsigned char taken[2048 + 8];
    memset(taken, 0, sizeof taken);
    for (uint32_t k = 0; k < 8u; ++k) {
        const bool w = (wide >> k) & 1u;
        const uint32_t before = incl.v[k] - own.v[k];
        for (uint32_t i = 0; i < visits[k]; ++i) {
            const uint32_t rank = w ? i * 8u : i;  // what the bin's counter held
            const uint32_t at = flat_item_slot(r, before, rank, w);
            const uint32_t want = split ? (w ? wide_before[k] + rank : wide_lanes + narrow_before[k] + rank) : visits_before[k] + i;
            const uint32_t width = split && w ? 8u : 1u;
            if (at != want || at + width > n_items || (width == 8u && (at & 7u) != 0u)) {
                printf("slot differs: bin %u visit %u at %u, plain %u (items %u)\n", k, i, at, want, n_items);
                return false;
            }
            for (uint32_t j = 0; j < width; ++j) {
                if (taken[at + j]) {
                    printf("slot %u taken twice\n", at + j);
                    return false;
                }
                taken[at + j] = 1;
            }
        }
    }
    for (uint32_t i = 0; i < n_items; ++i) {
        if (!taken[i]) {
            printf("slot %u of %u not taken\n", i, n_items);
            return false;
        }
    }
    return true;
}

static long check_prefix(int rounds) {
    long n = 0, splits = 0, fallbacks = 0;
    // the boundary: wide + narrow lanes == 256 (octets), == 257 (one lane per visit), and the largest totals of each field
    const uint32_t edge[][9] = {
        {31, 8, 0, 0, 0, 0, 0, 0, 0x01}, {31, 9, 0, 0, 0, 0, 0, 0, 0x01}, {8, 1, 4, 3, 9, 10, 1, 73, 0x15}, {8, 1, 4, 3, 9, 10, 1, 74, 0x15},
        {0, 0, 0, 0, 0, 0, 0, 32, 0x80}, {0, 0, 0, 0, 0, 0, 0, 33, 0x80}, {256, 0, 0, 0, 0, 0, 0, 0, 0x01}, {0, 0, 0, 0, 0, 0, 0, 256, 0x80},
        {256, 0, 0, 0, 0, 0, 0, 0, 0x00}, {0, 0, 0, 0, 0, 0, 0, 256, 0x00}, {32, 32, 32, 32, 32, 32, 32, 32, 0xFF}, {32, 32, 32, 32, 32, 32, 32, 32, 0x00},
        {0, 0, 0, 0, 0, 0, 0, 0, 0xFF}, {1, 0, 0, 0, 0, 0, 0, 0, 0x01}, {0, 0, 0, 0, 0, 0, 0, 1, 0x00}};
    for (const auto& e : edge) {
        uint32_t visits[8];
        for (int k = 0; k < 8; ++k) visits[k] = e[k];
        if (!check_round(visits, e[8])) return -1;
        n += 1;
    }
    {   // the two boundary cases are what they are meant to be
        const uint32_t a[8] = {31, 8, 0, 0, 0, 0, 0, 0}, b[8] = {31, 9, 0, 0, 0, 0, 0, 0};
        Row own;
        for (int i = 0; i < 16; ++i) own.v[i] = 0u;
        own.v[0] = flat_pack_bin(31u * 8u, true), own.v[1] = flat_pack_bin(a[1], false);
        const FlatRound ra = flat_round(flat_prefix8(own, RowShr{}).v[7]);
        own.v[1] = flat_pack_bin(b[1], false);
        const FlatRound rb = flat_round(flat_prefix8(own, RowShr{}).v[7]);
        if (!(ra.split && ra.n_items == 256u && !rb.split && rb.n_items == 40u)) {
            printf("boundary: 256 lanes split %d items %u, 257 lanes split %d items %u\n", int(ra.split), ra.n_items, int(rb.split), rb.n_items);
            return -1;
        }
    }
    for (int i = 0; i < rounds; ++i) {
        uint32_t visits[8], left = rnd() % 257u;  // at most 256 visits: one per ray of the workgroup
        const uint32_t wide = (i & 3) == 0 ? 0u : rnd() & 0xFFu;
        const uint32_t bins = 1u + rnd() % 8u;  // (few bins: large counts per bin)
        for (uint32_t k = 0; k < 8u; ++k) {
            visits[k] = (k < bins && left != 0u) ? rnd() % (left + 1u) : 0u;
            if (k + 1u == bins && (rnd() & 1u)) visits[k] = left;
            left -= visits[k];
        }
        if (rnd() & 1u) {  // bins in another order
            for (uint32_t k = 7u; k > 0u; --k) {
                const uint32_t j = rnd() % (k + 1u), t = visits[k];
                visits[k] = visits[j], visits[j] = t;
            }
        }
        if (!check_round(visits, wide)) return -1;
        uint32_t wl = 0u, nl = 0u;
        for (uint32_t k = 0; k < 8u; ++k) ((wide >> k) & 1u ? wl : nl) += ((wide >> k) & 1u) ? visits[k] * 8u : visits[k];
        (wl != 0u && wl + nl <= 256u ? splits : fallbacks) += 1;
        n += 1;
    }
    if (splits == 0 || fallbacks == 0) return -1;
    return n;
}

int main(int argc, char** argv) {
    const int draws = argc > 1 ? atoi(argv[1]) : 2000, rounds = argc > 2 ? atoi(argv[2]) : 200000;
    const long picks = check_picks(draws);
    if (picks < 0) return 1;
    const long prefixes = check_prefix(rounds);
    if (prefixes < 0) return 1;
    printf("%ld %ld\n", picks, prefixes);
    return 0;
}
