// tests/test_u8_division.py: every byte through the two-fma form of hiprz_u8_div.hpp against the division, bit for bit, and the
// count of bytes for which the bare product n * y is NOT the quotient (why the refinement is there).
// Prints "<bytes checked> <mismatches of the short form> <mismatches of the bare product>".
#include <cstdio>
#include <cstring>

#include "hiprz_u8_div.hpp"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    unsigned checked = 0, bad = 0, bare_bad = 0;
    for (unsigned b = 0; b < 256u; ++b) {
        volatile float n = float(b), d = 255.0f;  // volatile: the quotient is computed by the division, not folded
        const float want = n / d;
        if (bits(hiprz::u8_over_255_short(n)) != bits(want)) {
            std::printf("byte %u: short form %08x, division %08x\n", b, bits(hiprz::u8_over_255_short(n)), bits(want));
            bad += 1;
        }
        if (bits(hiprz::u8_over_255(n)) != bits(want)) bad += 1;  // whichever way RZ_U8_SHORT_DIV stands
        if (bits(n * hiprz::kRcp255) != bits(want)) bare_bad += 1;
        checked += 1;
    }
    std::printf("%u %u %u\n", checked, bad, bare_bad);
    return bad == 0 ? 0 : 1;
}
