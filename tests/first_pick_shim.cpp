// tests/test_first_pick.py: flat_pick_first of rayzath_amd/csrc/hiprz_flat_pick.hpp against a literal restatement, in a program of its
// own (g++ with ASan and UBSan).  Prints one line of counts; any difference ends it with a message and exit status 1.
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

// the one-by-one chain of the walk's candidate search: order[] = the leaf's instance ids in leaf order
static uint32_t chain_pick(const uint32_t (&order)[8], const float (&tm)[8], float far_, uint32_t& flat_mask, uint32_t& flat_next) {
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
// the restatement: the chain on copies, committed iff there is no candidate or the candidate's bit in `small` is set
static uint32_t first_pick(const uint32_t (&order)[8], const float (&tm)[8], float far_, uint32_t& flat_mask, uint32_t& flat_next, uint32_t small) {
    uint32_t m = flat_mask, n = flat_next;
    const uint32_t cand = chain_pick(order, tm, far_, m, n);
    if (cand != 0xFFFFFFFFu && ((small >> cand) & 1u) == 0u) return 0xFFFFFFFFu;
    flat_mask = m, flat_next = n;
    return cand;
}

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNan = std::numeric_limits<float>::quiet_NaN();
static const float kPool[] = {0.0f, -0.0f, kInf, -kInf, kNan, 1.0f, 1.0f, 2.0f, -1.0f, 0.5f, 3.402823466e+38f, 1.401298464e-45f, 1.00000012f};
// CLASS 0: every value from the pool (equal values, tm[k] == far, zeros of both signs, infinities, NaN); 1: small finite values with far
// taken from the tm half of the time (tm[k] == far without specials); 2: random bit patterns (any float, NaNs of every payload)
static float draw(int cls) {
    if (cls == 0) return kPool[rnd() % (sizeof kPool / sizeof kPool[0])];
    if (cls == 1) return float(int(rnd() % 17u) - 8) * 0.25f;
    const uint32_t u = rnd() << 16 ^ rnd();
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    const int draws = argc > 1 ? atoi(argv[1]) : 2;
    long n = 0, committed = 0, declined = 0, finished = 0, nan_seen = 0, equal_far = 0, followed = 0;
    for (uint32_t mask = 0; mask < 256u; ++mask) {
        for (uint32_t small = 0; small < 256u; ++small) {
            for (uint32_t next = 0; next <= 8u; ++next) {
                for (int cls = 0; cls < 3; ++cls) {
                    for (int d = 0; d < draws; ++d) {
                        float tm[8];
                        for (float& t : tm) t = draw(cls);
                        float far_ = draw(cls);
                        if (cls == 1 && (rnd() & 1u)) far_ = tm[rnd() & 7u];
                        uint32_t order[8], ids = 0u;  // instance ids of a leaf of at most 8: below 8, in any order, repeats allowed
                        for (uint32_t k = 0; k < 8u; ++k) order[k] = (k * 5u + (rnd() & 7u)) & 7u, ids = flat_pack_id(ids, k, order[k]);
                        uint32_t m0 = mask, n0 = next, m1 = mask, n1 = next;
                        const uint32_t want = first_pick(order, tm, far_, m0, n0, small);
                        const uint32_t got = flat_pick_first(ids, tm, far_, m1, n1, small);
                        if (want != got || m0 != m1 || n0 != n1) {
                            printf("first pick differs: mask %02x small %02x next %u far %08x tm", mask, small, next, bits(far_));
                            for (float t : tm) printf(" %08x", bits(t));
                            printf(": candidate %u / %u, mask %02x / %02x, next %u / %u (restatement / header)\n", want, got, m0, m1, n0, n1);
                            return 1;
                        }
                        // what flat_pick alone yields from the same state
                        uint32_t ma = mask, na = next;
                        const uint32_t alone = flat_pick(ids, tm, far_, ma, na);
                        if (got != kFlatNone) {  // committed: the candidate and the state are flat_pick's
                            committed += 1;
                            if (got != alone || m1 != ma || n1 != na || ((small >> got) & 1u) == 0u) {
                                printf("committed pick is not flat_pick's: mask %02x small %02x next %u: %u / %u\n", mask, small, next, got, alone);
                                return 1;
                            }
                        } else if (alone == kFlatNone) {  // no candidate at all: finished as flat_pick finishes it
                            finished += 1;
                            if (m1 != ma || n1 != na || m1 != 0u) {
                                printf("finished ray differs: mask %02x next %u: mask %02x / %02x next %u / %u\n", mask, next, m1, ma, n1, na);
                                return 1;
                            }
                        } else {  // declined: state untouched, and flat_pick after it yields what flat_pick alone yields
                            declined += 1;
                            if (m1 != mask || n1 != next) {
                                printf("declined pick touched the state: mask %02x -> %02x next %u -> %u\n", mask, m1, next, n1);
                                return 1;
                            }
                            const uint32_t then = flat_pick(ids, tm, far_, m1, n1);
                            if (then != alone || m1 != ma || n1 != na || ((small >> alone) & 1u) != 0u) {
                                printf("flat_pick behind a declined pick differs: mask %02x small %02x next %u: %u / %u\n", mask, small, next, then, alone);
                                return 1;
                            }
                            followed += 1;
                        }
                        n += 1;
                        for (float t : tm) nan_seen += t != t, equal_far += t == far_;
                    }
                }
            }
        }
    }
    // the draws reached what they are for
    if (committed == 0 || declined == 0 || finished == 0 || nan_seen == 0 || equal_far == 0 || followed != declined) {
        printf("draws: %ld committed, %ld declined, %ld finished, %ld NaN, %ld tm == far\n", committed, declined, finished, nan_seen, equal_far);
        return 1;
    }
    printf("%ld %ld %ld %ld\n", n, committed, declined, finished);
    return 0;
}
