// tests/test_pair_pick.py: rayzath_amd/csrc/hiprz_pair_pick.hpp against the one-by-one loop over two triangles, in a program of its own
// (g++ with ASan and UBSan).  Prints one line of counts; any difference ends it with a message and exit status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "hiprz_pair_pick.hpp"

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

// The leaf's loop as closest_in_mesh_stack runs it, on two triangles: within[k] = triangle k's barycentrics are inside it; the range test
// is tri_hit's, `t <= near || t >= far` rejects, and an accepted triangle's distance is the far end the next one meets.
static void one_by_one(const bool (&within)[2], const float (&t)[2], float near_, float& far_, uint32_t& winner) {
    winner = 0u;
    for (uint32_t k = 0; k < 2u; ++k) {
        if (!within[k]) continue;
        if (t[k] <= near_ || t[k] >= far_) continue;
        far_ = t[k];
        winner = k + 1u;
    }
}

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNan = std::numeric_limits<float>::quiet_NaN();
static const float kPool[] = {0.0f, -0.0f, kInf, -kInf, kNan, 1.0f, 1.0f, 2.0f, -1.0f, 0.5f, 3.402823466e+38f, 1.401298464e-45f, 1.00000012f};
// CLASS 0: every value from the pool (equal values, zeros of both signs, infinities, NaN); 1: small finite values, and half of the time a
// distance IS the near end, the far end or the other distance; 2: random bit patterns (any float, NaNs of every payload)
static float draw(int cls) {
    if (cls == 0) return kPool[rnd() % (sizeof kPool / sizeof kPool[0])];
    if (cls == 1) return float(int(rnd() % 17u) - 8) * 0.25f;
    const uint32_t u = rnd() << 16 ^ rnd();
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    const int draws = argc > 1 ? atoi(argv[1]) : 200000;
    long n = 0, won[3] = {0, 0, 0}, equal = 0, on_near = 0, on_far = 0, nan_seen = 0, zeros = 0;
    for (uint32_t mask = 0; mask < 4u; ++mask) {
        for (int cls = 0; cls < 3; ++cls) {
            for (int d = 0; d < draws; ++d) {
                float t[2] = {draw(cls), draw(cls)};
                float near_ = draw(cls), far_ = draw(cls);
                if (cls == 1 && (rnd() & 1u)) {
                    const uint32_t how = rnd() % 5u, k = rnd() & 1u;
                    if (how == 0u) t[1] = t[0];
                    else if (how == 1u) t[k] = near_;
                    else if (how == 2u) t[k] = far_;
                    else if (how == 3u) t[0] = t[1] = far_;
                    else t[0] = t[1] = near_;
                }
                const bool within[2] = {(mask & 1u) != 0u, (mask & 2u) != 0u};
                float want_far = far_;
                uint32_t want = 0u;
                one_by_one(within, t, near_, want_far, want);
                // what tri_hit2 hands over: inside the triangle and not at or before the near end
                const uint32_t inside = uint32_t(within[0] && !(t[0] <= near_)) | (uint32_t(within[1] && !(t[1] <= near_)) << 1);
                const PairPick got = pair_pick(inside, t[0], t[1], far_);
                if (got.winner != want || bits(got.far_) != bits(want_far)) {
                    printf("pair differs: mask %u t %08x %08x near %08x far %08x: winner %u / %u, far %08x / %08x (one by one / pair)\n", mask, bits(t[0]),
                           bits(t[1]), bits(near_), bits(far_), want, got.winner, bits(want_far), bits(got.far_));
                    return 1;
                }
                n += 1, won[want] += 1;
                equal += mask == 3u && t[0] == t[1] && want == 1u;   // equal distances: the first in leaf order won
                on_near += t[0] == near_ || t[1] == near_, on_far += t[0] == far_ || t[1] == far_;
                nan_seen += t[0] != t[0] || t[1] != t[1] || far_ != far_ || near_ != near_;
                zeros += (bits(t[0]) << 1) == 0u || (bits(t[1]) << 1) == 0u;
            }
        }
    }
    // the draws reached what they are for
    if (won[0] == 0 || won[1] == 0 || won[2] == 0 || equal == 0 || on_near == 0 || on_far == 0 || nan_seen == 0 || zeros == 0) {
        printf("pair draws: winners %ld %ld %ld, %ld equal distances, %ld on the near end, %ld on the far end, %ld NaN, %ld zeros\n", won[0], won[1],
               won[2], equal, on_near, on_far, nan_seen, zeros);
        return 1;
    }
    printf("%ld\n", n);
    return 0;
}
