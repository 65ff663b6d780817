// The Montgomery form of a machine word: shared by the typed-column decoder (fr_ntt.hip, k_fr_from_typed) and the integer ALU
// columns (fr_int.hip, k_fr_int; fr_alu.hip, k_fr_alu), so that every translation unit encodes with one body.
#pragma once
#include "fr29.hip.h"

// x * 2^261 mod r for x < 2^64, below 2r: x has three limbs, so a Montgomery product of radix 2^87 by 2^(261 + 87) mod r
// does it -- 27 + 24 mads where fr9_to_mont spends 81 + 72.  (x C + q r) / 2^87 < (2^64 + 2^87) r / 2^87 < 2r; a column sum
// is at most six products below 2^58.  Modelled limb by limb against x * 2^261 % r over the edges and 2 x 10^4 random x.
FR9_TABLE(fr9_2_348, 0x1c74a235u, 0x1cebd299u, 0x0150fcf8u, 0x18886c4cu, 0x162c0a9du, 0x06cbaa5fu, 0x17bd1efeu, 0x06f2bf4bu, 0x0032f10cu)
KZG_DEV void fr9_mont_from_u64(fr9_t& r, uint64_t x) {
    const uint32_t a[3] = {(uint32_t)x & FR9_MASK, (uint32_t)(x >> 29) & FR9_MASK, (uint32_t)(x >> 58)};
    uint32_t q[3];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = k - i;
            if (j >= 0 && j < 9) acc += (uint64_t)a[i] * fr9_2_348(j);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = k - i;
            if (i < k && j >= 1 && j < 9) acc += (uint64_t)q[i] * fr9_r(j);
        }
        if (k < 3) {
            q[k] = (0u - (uint32_t)acc) & FR9_MASK;
            acc += q[k];
        } else {
            r.l[k - 3] = (uint32_t)acc & FR9_MASK;
        }
        acc >>= 29;
    }
    r.l[8] = (uint32_t)acc;
}

// ---- a cell in, a machine word out: the two ends of every integer ALU kernel (fr_int.hip, fr_alu.hip)
// the canonical integer of the cell at p: its low 64 bits; *high <- whether a bit at or above 2^64 is set
KZG_DEV uint64_t int_load(const uint32_t* p, bool* high) {
    fr9_t v;
    uint32_t w[8];
    fr9_load(v, p);
    fr9_from_mont(v, v);
    fr9_to_words(w, v);
    *high = (w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;
    return ((uint64_t)w[1] << 32) | w[0];
}
KZG_DEV void int_store(uint32_t* p, uint64_t x) {
    fr9_t v;
    fr9_mont_from_u64(v, x);
    fr9_canon(v, v);
    fr9_store(p, v);
}
// int_store with a sign: the cell of x, or where neg (then x is in [1, 2^64)) of -x, which is r - x: the convention of the typed
// i64 columns (fr_wide.hip's carries).  One encoder; the negation acts on the canonical element before the store
KZG_DEV void int_store_signed(uint32_t* p, uint64_t x, bool neg) {
    fr9_t v;
    fr9_mont_from_u64(v, x);
    fr9_canon(v, v);
    int32_t br = 0;   // (the residue of x is not zero: r - v is canonical)
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int32_t d = (int32_t)fr9_r(i) - (int32_t)v.l[i] + br;
        br = d >> 29;
        v.l[i] = neg ? ((i < 8) ? ((uint32_t)d & FR9_MASK) : (uint32_t)d) : v.l[i];
    }
    fr9_store(p, v);
}
