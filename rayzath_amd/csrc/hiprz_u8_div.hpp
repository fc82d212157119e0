// hiprz_u8_div.hpp — a byte over 255 (Color -> ColorF: from_u8, fetch_r8 in hiprz_device.hpp) without the division's expansion.
// With y = the float nearest to 1/255, n * y is the correctly rounded n / 255.0f for only 130 of the 256 bytes; one refinement —
// the residual n - 255 q from an fma (exact: q is within an ulp of the quotient), times y, added to q in a second fma — gives the
// correctly rounded quotient for all 256.  Two fmas are the whole of it: they are spelled as fmas, so -ffp-contract=off leaves
// them alone.  No HIP header: tests/test_u8_division.py compiles it with g++ and checks every byte against `/`; on the device
// hiprz_selftest does the same.
#pragma once
#include <stdint.h>

#ifndef RZ_DEV  // (hiprz_device.hpp defines it for the device before it includes this file)
#define RZ_DEV inline
#endif

#ifndef RZ_U8_SHORT_DIV  // 0: from_u8 and fetch_r8 divide by 255.0f
#define RZ_U8_SHORT_DIV 1
#endif

namespace hiprz {

constexpr float kRcp255 = 0x1.010102p-8f;  // the float nearest to 1/255

// n = float(a byte), 0 .. 255
RZ_DEV float u8_over_255_short(float n) {
    const float q = n * kRcp255;
    return __builtin_fmaf(__builtin_fmaf(-255.0f, q, n), kRcp255, q);
}
RZ_DEV float u8_over_255(float n) {
#if RZ_U8_SHORT_DIV
    return u8_over_255_short(n);
#else
    return n / 255.0f;
#endif
}

}  // namespace hiprz
