// fr_poseidon2.hip -- Fr-side kernels, part 22: the Poseidon2 permutation columns of kzg_rows_commit_poseidon2.  Over Fr with the
// S-box x^5 and the CALLER's constants, t in {2, 3, 4, 8}:
//   s <- E(s); R_F / 2 full rounds; R_P partial rounds; R_F / 2 full rounds, where
//   a full round     s_i += rc_full[rho' t + i], s_i <- s_i^5 for every i, s <- E(s)   (rho' counts the full rounds of both halves)
//   a partial round  s_0 += rc_partial[rho''], s_0 <- s_0^5, s <- I(s)
//   E  t = 2, 3: y_i = s_i + sum_j s_j; t = 4: y = M4 s; t = 8: u = (M4 s[0..3], M4 s[4..7]), y_{4k+j} = u_{4k+j} + u_j + u_{4+j}
//   I  y_i = diag_i s_i + sum_j s_j
// E has NO field product (M4 is the addition chain of p2_m4), I has t.  Source columns lie as evaluation vectors of T elements of
// 8 words, Montgomery, CANONICAL (the forward transform ends in fr9_reduce).
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE body k_fr_poseidon2<t> for the three unit forms, the table
//   PosTab of k_fr_poseidon<t> as it is: the state is t fr9_t in registers, indexed by constants only; the round loop's trip
//   counts are uniform.  E is straight-line, and I up to t = 4; the S-boxes of a round, and the t products of I at t = 8, are
//   REAL loops (#pragma unroll 1) whose element is picked and put back by uniform selects, as in fr_poseidon.hip.  No
//   instantiation has scratch: 83 / 100 / 126 / 222 VGPRs, no AGPRs, 5 / 4 / 4 / 2 waves per SIMD.
//     a ROW unit     one lane per row t' < n: the permutation, then one store per output column;
//     a check        the same lane compares instead of storing (derive_count, expr_first);
//     a ROUNDS unit  one lane per block of P >= R + 2 rows, floor(n / P) lanes: the input at the block's row 0, E(input) at row 1,
//                    the state behind round rho at row 2 + rho; the rows between the blocks were zeroed by the caller.
//   The constants -- t R_F full-round constants, R_P partial-round constants, t diagonal entries, the unit's t immediates -- come
//   from a device buffer as 8 words of a canonical integer each and are converted to Montgomery form into LDS once per
//   workgroup: (t R_F + R_P + 2 t) x 36 bytes of dynamic LDS, at most 9792.
//   Operand classes (fr29.hip.h), written (V, L): the value is below V r, limbs 0 .. 7 are at most L (2^29 - 1); limb 8 carries
//   the excess and stays below 2^29 while V <= 64.  A lazy value needs L <= 4 (limbs below 2^31) and V < 64.
//     THE INVARIANT: the state is canonical, (1, 1), at the head of every round and at every store: a loaded cell, an immediate
//     from LDS, or fr9_reduce's output.
//     constants      u = s + rc: (2, 2).  Under an S-box u is normalised (a legal SECOND operand; u u < 4 r^2 against the 70 r^2 a
//                    product takes); u^2, u^4 and u^5 = u^4 u are products' outputs (2, 1); fr9_canon makes u^5 canonical (1, 1),
//                    so that both linear layers add canonical-sized terms only.
//     E, t = 2, 3    sum (3, 3); y_i = s_i + sum (4, 4).
//     E, t = 4       p2_m4's outputs (16, 4): the bounds beside its chain.
//     E, t = 8       the eight u are normalised to (16, 1); y = 2 u_own + u_other: (48, 3).
//     I              sum: t canonical terms, normalised after every third and at the end: (8, 1), never above L = 4 on the
//                    way; diag_i s_i: s_i canonical the first operand, diag_i canonical from LDS the second, the product (2, 1);
//                    y_i = product + sum (10, 2).
//   Every y is inside the (64, 4) that fr9_reduce takes, which closes with fr9_canon.  Every stored cell is canonical, every
//   store is a vector store (fr9_store: two 16-byte stores).
// Bound: a permutation is R_F 3 t + R_P (3 + t) field products per lane -- 408 at t = 3, (8, 56); 819 at t = 8, (8, 57) -- against
// 32 t B read and 32 n_out B written (ROUNDS: 32 t (R + 2) B written): the multiplier.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

KZG_DEV void p2_lds(fr9_t& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
}

// x <- s[i] and s[i] <- x for a uniform i, limb by limb through selects.  THE CONSTRAINT: the state must stay in registers, so
// nothing may index s at run time and no whole element may be copied under an `if`: the compiler turns such a copy into a
// choice between POINTERS into s, and an array whose address is chosen at run time lives in private memory (scratch)
template <int TW>
KZG_DEV void p2_pick(fr9_t& x, const fr9_t* s, uint32_t i) {
    x = s[0];
#pragma unroll
    for (int k = 1; k < TW; k++)
#pragma unroll
        for (int l = 0; l < 9; l++) x.l[l] = k == (int)i ? s[k].l[l] : x.l[l];
}
template <int TW>
KZG_DEV void p2_put(fr9_t* s, uint32_t i, const fr9_t& x) {
#pragma unroll
    for (int k = 0; k < TW; k++)
#pragma unroll
        for (int l = 0; l < 9; l++) s[k].l[l] = k == (int)i ? x.l[l] : s[k].l[l];
}

// x <- M4 x, M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]], by the addition chain; x canonical (1, 1) in, lazy out
KZG_DEV void p2_m4(fr9_t& x0, fr9_t& x1, fr9_t& x2, fr9_t& x3) {
    fr9_t a, b, c, d, e, f;
    fr9_add(a, x0, x1);   // a = x0 + x1                (2, 2)
    fr9_add(b, x2, x3);   // b = x2 + x3                (2, 2)
    fr9_add(c, x1, x1);
    fr9_add(c, c, b);     // c = 2 x1 + b               (4, 4)
    fr9_add(d, x3, x3);
    fr9_add(d, d, a);     // d = 2 x3 + a               (4, 4)
    fr9_norm(c, c);       //                            (4, 1)
    fr9_norm(d, d);       //                            (4, 1)
    fr9_add(a, a, a);     // 2 a                        (4, 4)
    fr9_add(b, b, b);     // 2 b                        (4, 4)
    fr9_norm(a, a);       //                            (4, 1)
    fr9_norm(b, b);       //                            (4, 1)
    fr9_add(e, b, b);
    fr9_add(e, e, d);     // e = 4 b + d                (12, 3)
    fr9_add(f, a, a);
    fr9_add(f, f, c);     // f = 4 a + c                (12, 3)
    fr9_add(x0, d, f);    // d + f                      (16, 4)
    x1 = f;               //                            (12, 3)
    fr9_add(x2, c, e);    // c + e                      (16, 4)
    x3 = e;               //                            (12, 3)
}

// s <- E(s): s canonical in and out
template <int TW>
KZG_DEV void p2_external(fr9_t* s) {
    if constexpr (TW == 2 || TW == 3) {
        fr9_t sum;
        fr9_add(sum, s[0], s[1]);
        if constexpr (TW == 3) fr9_add(sum, sum, s[2]);   // (3, 3)
#pragma unroll
        for (int i = 0; i < TW; i++) {
            fr9_add(s[i], s[i], sum);                     // (4, 4)
            fr9_reduce(s[i], s[i]);
        }
    } else if constexpr (TW == 4) {
        p2_m4(s[0], s[1], s[2], s[3]);                    // (16, 4)
#pragma unroll
        for (int i = 0; i < 4; i++) fr9_reduce(s[i], s[i]);
    } else {
        static_assert(TW == 8, "t is 2, 3, 4 or 8");
        p2_m4(s[0], s[1], s[2], s[3]);
        p2_m4(s[4], s[5], s[6], s[7]);
#pragma unroll
        for (int i = 0; i < 8; i++) fr9_norm(s[i], s[i]);   // u: (16, 1)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            fr9_t v;
            fr9_add(v, s[j], s[4 + j]);                   // u_j + u_{4+j}   (32, 2)
            fr9_add(s[j], s[j], v);                       //                 (48, 3)
            fr9_add(s[4 + j], s[4 + j], v);               //                 (48, 3)
            fr9_reduce(s[j], s[j]);
            fr9_reduce(s[4 + j], s[4 + j]);
        }
    }
}

// s <- I(s): s canonical in and out; diag: t canonical scalars of 9 limbs in LDS
template <int TW>
KZG_DEV void p2_internal(fr9_t* s, const uint32_t* diag) {
    fr9_t sum = s[0];
#pragma unroll
    for (int j = 1; j < TW; j++) {
        fr9_add(sum, sum, s[j]);                          // at most (j + 1, 4)
        if (j % 3 == 2) fr9_norm(sum, sum);               //         (j + 1, 1)
    }
    if constexpr (TW % 3 != 0) fr9_norm(sum, sum);        // (8, 1)
    if constexpr (TW <= 4) {
#pragma unroll
        for (int i = 0; i < TW; i++) {
            fr9_t m, p;
            p2_lds(m, diag + 9 * i);
            fr9_mul(p, s[i], m);                          // (2, 1)
            fr9_add(p, p, sum);                           // (10, 2)
            fr9_reduce(s[i], p);
        }
    } else {
        // (t = 8: eight products and reductions in line exceed what the compiler unrolls under the pragma, and a loop it does
        // not unroll indexes s at run time: scratch.  Hence a real loop, s_i picked and put back by uniform selects)
#pragma unroll 1
        for (uint32_t i = 0; i < TW; i++) {
            fr9_t m, p, x;
            p2_pick<TW>(x, s, i);
            p2_lds(m, diag + 9 * i);
            fr9_mul(p, x, m);                             // (2, 1)
            fr9_add(p, p, sum);                           // (10, 2)
            fr9_reduce(p, p);
            p2_put<TW>(s, i, p);
        }
    }
}

// T a power of two, n <= T; every slot, col and exp of the unit either its escape value or the index of a vector below src /
// out (the launcher's and its caller's checks).  Workgroups past the unit's last lane leave at once (before any barrier);
// lanes past it inside the last workgroup read nothing and store nothing; they still walk the two reductions.
template <int TW>
__global__ void __launch_bounds__(256) k_fr_poseidon2(const PosTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    extern __shared__ uint32_t lds[];   // [t R_F] rc_full, [R_P] rc_partial, [t] diag, [t] the unit's immediates: 9 limbs each
    const PosUnit& U = tab.u[blockIdx.y];
    const uint32_t R = tab.full + tab.partial, half = tab.full / 2, nrf = TW * tab.full, nsh = nrf + tab.partial + TW, nc = nsh + TW;
    const bool rounds = U.mode == POS_ROUNDS;
    const uint64_t lanes = rounds ? n / U.period : n;
    if ((uint64_t)blockIdx.x * blockDim.x >= lanes) return;
    for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) {
        const uint32_t at = k < nsh ? k : k + blockIdx.y * TW;
        const uint4* q = reinterpret_cast<const uint4*>(tab.cst + 8 * (size_t)at);
        const uint4 a = q[0], b = q[1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        fr9_t c;
        fr9_from_words(c, w);
        fr9_to_mont(c, c);
#pragma unroll
        for (int i = 0; i < 9; i++) lds[9 * k + i] = c.l[i];
    }
    __syncthreads();
    const uint32_t *rcp = lds + 9 * nrf, *diag = rcp + 9 * tab.partial, *imm = diag + 9 * TW;
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool differs = false;
    if (v < lanes) {
        const uint64_t row = rounds ? v * U.period : v;
        fr9_t s[TW];
#pragma unroll
        for (int i = 0; i < TW; i++) {
            if (U.slot[i] == POS_IMM) p2_lds(s[i], imm + 9 * i);
            else fr9_load(s[i], tab.src + 8 * (U.slot[i] * T + row));
            if (rounds) fr9_store(U.out + 8 * (i * T + row), s[i]);
        }
        p2_external<TW>(s);
        if (rounds) {
#pragma unroll
            for (int i = 0; i < TW; i++) fr9_store(U.out + 8 * (i * T + row + 1), s[i]);
        }
        for (uint32_t rho = 0; rho < R; rho++) {
            const bool full = rho < half || rho >= half + tab.partial;
            if (full) {
                const uint32_t* rc = lds + 9 * TW * (rho < half ? rho : rho - tab.partial);
#pragma unroll
                for (int i = 0; i < TW; i++) {
                    fr9_t c;
                    p2_lds(c, rc + 9 * i);
                    fr9_add(s[i], s[i], c);               // (2, 2)
                }
            } else {
                fr9_t c;
                p2_lds(c, rcp + 9 * (rho - half));
                fr9_add(s[0], s[0], c);                   // (2, 2)
            }
            const uint32_t n_sbox = full ? TW : 1;
#pragma unroll 1
            for (uint32_t i = 0; i < n_sbox; i++) {   // (a real loop: one S-box in flight, s_i picked and put back by selects)
                fr9_t u, p;
                p2_pick<TW>(u, s, i);
                fr9_norm(u, u);
                fr9_mul(p, u, u);
                fr9_mul(p, p, p);
                fr9_mul(p, p, u);
                fr9_canon(p, p);                          // (1, 1)
                p2_put<TW>(s, i, p);
            }
            if (full) p2_external<TW>(s);
            else p2_internal<TW>(s, diag);
            if (rounds) {
#pragma unroll
                for (int i = 0; i < TW; i++) fr9_store(U.out + 8 * (i * T + row + rho + 2), s[i]);
            }
        }
        if (!rounds) {
#pragma unroll
            for (int i = 0; i < TW; i++) {
                const uint32_t c = U.col[i];
                if (c == POS_NO_COL) continue;
                if (U.out) {
                    fr9_store(U.out + 8 * (c * T + row), s[i]);
                } else {
                    const uint4* q = reinterpret_cast<const uint4*>(tab.src + 8 * (U.exp[c] * T + row));
                    const uint4 a = q[0], b = q[1];
                    uint32_t w[8];
                    fr9_to_words(w, s[i]);
                    differs |= ((w[0] ^ a.x) | (w[1] ^ a.y) | (w[2] ^ a.z) | (w[3] ^ a.w) | (w[4] ^ b.x) | (w[5] ^ b.y) | (w[6] ^ b.z) |
                                (w[7] ^ b.w)) != 0;
                }
            }
        }
    }
    derive_count(differs, st + blockIdx.y);
    expr_first(differs, st + tab.n_units + blockIdx.y);
}

uint32_t poseidon2_cst_words(uint32_t t, uint32_t full, uint32_t partial, uint32_t n_units) {
    return 8 * (t * full + partial + t + t * n_units);
}

void launch_poseidon2(hipStream_t s, const PosTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    const uint32_t t = tab.t, R = tab.full + tab.partial;
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || (t != 2 && t != 3 && t != 4 && t != 8) || tab.full < 2 ||
        (tab.full & 1) || R > POS_MAX_ROUNDS || tab.n_units == 0 || tab.n_units > POS_MAX_UNITS || !tab.src || !tab.cst)
        return;
    uint64_t lanes = 0;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const PosUnit& U = tab.u[u];
        const bool rounds = U.mode == POS_ROUNDS;
        if ((!rounds && U.mode != POS_ROW) || (rounds && (U.period < R + 2 || !U.out))) return;
        for (uint32_t i = 0; i < t; i++) {
            if (U.slot[i] != POS_IMM && U.slot[i] >= POLY_MAX_ROWS) return;
            if (!rounds && U.col[i] != POS_NO_COL && (U.col[i] >= t || (!U.out && U.exp[U.col[i]] >= POLY_MAX_ROWS))) return;
        }
        const uint64_t l = rounds ? n / U.period : n;
        lanes = l > lanes ? l : lanes;
    }
    if (!lanes) return;   // (only ROUNDS units, each with a period above n: their zeroed columns are the result)
    const dim3 grid(nblk(lanes, 256), tab.n_units);
    const size_t smem = (size_t)(t * tab.full + tab.partial + 2 * t) * 36;
    auto* sp = reinterpret_cast<unsigned long long*>(stats);
    switch (t) {
    case 2: k_fr_poseidon2<2><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 3: k_fr_poseidon2<3><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 4: k_fr_poseidon2<4><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    default: k_fr_poseidon2<8><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    }
}
