// The library's device-side Fr inversion (one lane), shared by the grand product (fr_prod.hip) and the quotient (fr_quot.hip).
#pragma once
#include "fr_kernels.hip.h"

// a^-1 mod r of a canonical integer a != 0 by the binary extended Euclid (HAC 14.61): u, v shrink by halving and
// subtracting, x1, x2 follow mod r.  32-bit adds and shifts only -- ~760 steps of ~35 instructions for a random a, against
// ~330 dependent products (~70 000 instructions) for the Fermat power a^(r-2).  One lane; the bound of 1100 steps covers
// the worst case (<= 510 halvings, each subtraction is followed by one).
KZG_DEV void w8_shr1(uint32_t* a, uint32_t top) {
#pragma unroll
    for (int i = 0; i < 7; i++) a[i] = (a[i] >> 1) | (a[i + 1] << 31);
    a[7] = (a[7] >> 1) | (top << 31);
}
KZG_DEV void w8_half_mod(uint32_t* x, const uint32_t* r) {   // x <- x / 2 mod r (x < r < 2^255)
    uint32_t c = 0;
    if (x[0] & 1u) c = bi_add<8>(x, x, r);
    w8_shr1(x, c);
}
KZG_DEV void w8_sub_mod(uint32_t* x, const uint32_t* y, const uint32_t* r) {   // x <- x - y mod r
    if (bi_sub<8>(x, x, y)) (void)bi_add<8>(x, x, r);
}
KZG_DEV bool w8_is_one(const uint32_t* a) {
    uint32_t t = a[0] ^ 1u;
#pragma unroll
    for (int i = 1; i < 8; i++) t |= a[i];
    return t == 0;
}
// Montgomery form in, Montgomery form out; false (and zero out) for a == 0
KZG_DEV bool fr9_inv(fr9_t& out, const fr9_t& a_mont_lazy) {
    constexpr uint32_t RW[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    uint32_t r[8], u[8], v[8], x1[8], x2[8];
    fr9_t a;
    fr9_from_mont(a, a_mont_lazy);
    fr9_to_words(u, a);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r[i] = RW[i];
        v[i] = RW[i];
        x1[i] = i == 0 ? 1u : 0u;
        x2[i] = 0u;
    }
    if (bi_is_zero<8>(u)) {
        fr9_zero(out);
        return false;
    }
    for (int it = 0; it < 1100 && !w8_is_one(u) && !w8_is_one(v); it++) {
        if (!(u[0] & 1u)) {
            w8_shr1(u, 0);
            w8_half_mod(x1, r);
        } else if (!(v[0] & 1u)) {
            w8_shr1(v, 0);
            w8_half_mod(x2, r);
        } else if (bi_ge<8>(u, v)) {
            (void)bi_sub<8>(u, u, v);
            w8_sub_mod(x1, x2, r);
        } else {
            (void)bi_sub<8>(v, v, u);
            w8_sub_mod(x2, x1, r);
        }
    }
    fr9_t y;
    fr9_from_words(y, w8_is_one(u) ? x1 : x2);
    fr9_to_mont(out, y);
    return true;
}
