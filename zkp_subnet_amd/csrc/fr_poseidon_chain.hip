// fr_poseidon_chain.hip -- Fr-side kernels, part 21: the Poseidon sponge and Merkle-path chains of kzg_rows_commit_poseidon_chain.
// The permutation is fr_poseidon.hip's (the plain Hades schedule over Fr, S-box x^5, the caller's constants); what is new is the
// CARRY from one block of P rows into the next: a SPONGE block that continues adds its cells to the output of the block before,
// a PATH block that continues hashes one element of that output (the digest) among the level's siblings, at the child position
// the row's pos cell names.  Source columns lie as evaluation vectors of T elements of 8 words, Montgomery, CANONICAL.
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE body k_fr_poseidon_chain<t>; the constants are staged into
//   LDS once per workgroup exactly as k_fr_poseidon stages them ((t R + t t + t) x 36 bytes of dynamic LDS, at most 44064).
//   One lane per BLOCK, nb = floor(n / P) lanes: the lane of block b reads the block's start cell; where b continues a segment
//   it leaves at once; where b starts one (b = 0, no start column, or a start cell that is not zero) it walks the segment block
//   by block, reading the next block's start cell after each permutation, until the next start or the last block -- the scheme
//   of fr_keccak.hip's ROUNDS unit.  A segment is SERIAL: its length times one permutation's latency is the call's time,
//   whatever the number of segments up to the device's lanes (DESIGN.md has the measure, and what it left unexplained).  No
//   barrier follows the one behind the constants.
//   The state is t fr9_t in registers, indexed by constants only.  The round is pos_round below: a second copy of the round of
//   k_fr_poseidon (fr_poseidon.hip stays byte for byte as it is: DESIGN.md says why), the S-boxes and the rows of M REAL loops
//   whose element is picked and put back by uniform selects.  The sponge's carry is an unrolled loop over the t elements; the
//   path's arrangement is an unrolled loop over the a = t - 1 children whose three candidates (the sibling before, the running
//   digest, the sibling behind) are chosen per limb by PER-LANE selects on the position; the digest is picked out of the state
//   by a uniform select.  No instantiation has scratch (DESIGN.md has the figures).
//   Operand classes (fr29.hip.h; the comment at the head of fr_poseidon.hip).  The state is canonical at the head of every
//   round: a loaded cell, an immediate from LDS, fr9_reduce's output -- or the carry out_prev + cell: both canonical, the sum is
//   below 2 r with limbs below 2^30, fr9_norm makes it N class and fr9_canon canonical, BEFORE the round constants are added (and
//   before a flat in column stores it).  Every stored cell is canonical, every store is a vector store (fr9_store).
//   The pos cell is read as its whole canonical integer (int_load: one product): at or above a = t - 1 it is position 0 and
//   counted, once per block, by the lane that walks the block.  Statistics are plain atomics of the walking lanes.
// Bound: a permutation is R_F (3 t + t^2) + R_P (3 + t^2) field products on ONE lane; a segment of L blocks is L of them in a
// row.  Traffic is nothing beside it.
#include <cstring>

#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

KZG_DEV void pch_lds(fr9_t& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
}
// the cell at p is not zero (a canonical cell is zero where its words are)
KZG_DEV bool pch_nonzero(const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0;
}
// the canonical element v differs from the cell at p
KZG_DEV bool pch_differs(const uint32_t* p, const fr9_t& v) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    uint32_t w[8];
    fr9_to_words(w, v);
    return ((w[0] ^ a.x) | (w[1] ^ a.y) | (w[2] ^ a.z) | (w[3] ^ a.w) | (w[4] ^ b.x) | (w[5] ^ b.y) | (w[6] ^ b.z) | (w[7] ^ b.w)) != 0;
}

// One round on the canonical state s: the constants at rc (t of them), the S-box on every element (full) or on element 0, the
// matrix at mds; element i of the new state goes to trace + 8 i T as well where trace is not null.  The round of k_fr_poseidon
template <int TW>
KZG_DEV void pos_round(fr9_t (&s)[TW], const uint32_t* rc, const uint32_t* mds, bool full, uint32_t* trace, uint64_t T) {
    fr9_t x[TW];
#pragma unroll
    for (int i = 0; i < TW; i++) {
        fr9_t c;
        pch_lds(c, rc + 9 * i);
        fr9_add(x[i], s[i], c);
    }
    const uint32_t n_sbox = full ? TW : 1;
#pragma unroll 1
    for (uint32_t i = 0; i < n_sbox; i++) {   // (a real loop: one S-box in flight, x_i picked and put back by selects)
        fr9_t u, p;
        u = x[0];
#pragma unroll
        for (int k = 1; k < TW; k++)
            if (k == (int)i) u = x[k];
        fr9_norm(u, u);
        fr9_mul(p, u, u);
        fr9_mul(p, p, p);
        fr9_mul(p, p, u);
#pragma unroll
        for (int k = 0; k < TW; k++)
            if (k == (int)i) x[k] = p;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < TW; i++) {   // (a real loop: the row of M is read where it is used, and the code is one row's)
        const uint32_t* mrow = mds + 9 * TW * i;
        fr9_t acc, m, p;
        pch_lds(m, mrow);
        fr9_mul(acc, x[0], m);
#pragma unroll
        for (int j = 1; j < TW; j++) {
            pch_lds(m, mrow + 9 * j);
            fr9_mul(p, x[j], m);
            fr9_add(acc, acc, p);
            if (j % 3 == 2 && j + 1 < TW) fr9_norm(acc, acc);
        }
        fr9_reduce(acc, acc);
#pragma unroll
        for (int k = 0; k < TW; k++)
            if (k == (int)i) s[k] = acc;      // (i is uniform: a select per limb, the state stays in registers)
        if (trace) fr9_store(trace + 8 * (i * T), acc);
    }
}

// T a power of two, n <= T; every slot, col, start, pos, digest and exp of the unit either its escape value or inside its range
// (the launcher's and its caller's checks).  Workgroups past the unit's last block leave at once (before the barrier); lanes
// past it, and lanes whose block continues a segment, leave behind it
template <int TW>
__global__ void __launch_bounds__(256) k_fr_poseidon_chain(const PchTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    extern __shared__ uint32_t lds[];   // [t R] rc, [t t] M, [t] the unit's immediates: 9 limbs each
    const PchUnit& U = tab.u[blockIdx.y];
    const uint32_t R = tab.full + tab.partial, half = tab.full / 2, nrc = TW * R, nc = nrc + TW * TW + TW;
    const uint64_t P = U.period, nb = n / P;
    if ((uint64_t)blockIdx.x * blockDim.x >= nb) return;
    for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) {
        const uint32_t at = k < nrc + TW * TW ? k : k + blockIdx.y * TW;
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
    const uint32_t *mds = lds + 9 * nrc, *imm = mds + 9 * TW * TW;
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nb) return;
    const uint32_t* start = U.start == PCH_NONE ? nullptr : tab.src + 8 * (uint64_t)U.start * T;
    if (v != 0 && start && !pch_nonzero(start + 8 * v * P)) return;   // (the lane of the segment's first block walks this one)
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const bool path = U.mode == PCH_PATH, trace = U.layout == PCH_TRACE;
    uint32_t bad = 0, miss = 0;
    uint64_t first_bad = ~0ull, first_miss = ~0ull;
    fr9_t s[TW];
    bool cont = false;   // the block continues the one before: s holds that block's output
    for (uint64_t b = v;;) {
        const uint64_t row = b * P;
        if (path) {
            if constexpr (TW >= 3) {
                bool high;
                uint64_t p = int_load(tab.src + 8 * ((uint64_t)U.pos * T + row), &high);
                if (high || p >= (uint64_t)(TW - 1)) {
                    p = 0;
                    bad++;
                    first_bad = first_bad < row ? first_bad : row;
                }
                fr9_t cur, prev, nxt;
                if (cont) {
                    cur = s[0];
#pragma unroll
                    for (int k = 1; k < TW; k++)
                        if (k == (int)U.digest) cur = s[k];   // (uniform)
                } else if (U.slot[1] == POS_IMM) {
                    pch_lds(cur, imm + 9);
                } else {
                    fr9_load(cur, tab.src + 8 * ((uint64_t)U.slot[1] * T + row));
                }
                if (U.slot[0] == POS_IMM) pch_lds(s[0], imm);
                else fr9_load(s[0], tab.src + 8 * ((uint64_t)U.slot[0] * T + row));
                prev = cur;
#pragma unroll
                for (int k = 0; k < TW - 1; k++) {   // child k: the sibling before it, the digest, or the sibling behind it
                    if (k < TW - 2) fr9_load(nxt, tab.src + 8 * ((uint64_t)U.slot[2 + k] * T + row));
                    else nxt = cur;
                    const bool below = (uint64_t)k > p, here = (uint64_t)k == p;
#pragma unroll
                    for (int l = 0; l < 9; l++) s[1 + k].l[l] = below ? prev.l[l] : (here ? cur.l[l] : nxt.l[l]);
                    prev = nxt;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TW; i++) {
                if (U.slot[i] == POS_IMM) {
                    if (!cont) pch_lds(s[i], imm + 9 * i);   // (a tag or capacity immediate enters once per segment)
                } else {
                    fr9_t c;
                    fr9_load(c, tab.src + 8 * ((uint64_t)U.slot[i] * T + row));
                    if (cont) {   // out_prev + cell: two canonical values, back to canonical before the constants are added
                        fr9_add(c, s[i], c);
                        fr9_norm(c, c);
                        fr9_canon(c, c);
                    }
                    s[i] = c;
                }
            }
        }
        if (U.out) {
#pragma unroll
            for (int i = 0; i < TW; i++) {
                const uint32_t c = trace ? (uint32_t)i : U.col[i];
                if (c != PCH_NONE) fr9_store(U.out + 8 * ((uint64_t)c * T + row), s[i]);
            }
        }
        for (uint32_t rho = 0; rho < R; rho++)
            pos_round<TW>(s, lds + 9 * (rho * TW), mds, rho < half || rho >= half + tab.partial,
                          trace ? U.out + 8 * (row + rho + 1) : nullptr, T);
        if (U.out && !trace) {
#pragma unroll
            for (int i = 0; i < TW; i++) {
                const uint32_t c = U.col[POS_MAX_T + i];
                if (c != PCH_NONE) fr9_store(U.out + 8 * ((uint64_t)c * T + row), s[i]);
            }
        }
        const uint64_t nx = b + 1;
        if (nx >= nb || !start || pch_nonzero(start + 8 * nx * P)) {   // the segment's last block
            if (U.exp != PCH_NONE) {
                fr9_t d = s[0];
#pragma unroll
                for (int k = 1; k < TW; k++)
                    if (k == (int)U.digest) d = s[k];
                if (pch_differs(tab.src + 8 * ((uint64_t)U.exp * T + row), d)) {
                    miss = 1;
                    first_miss = row;
                }
            }
            break;
        }
        b = nx;
        cont = true;
    }
    atomicAdd(st + u, 1ull);
    if (bad) {
        atomicAdd(st + nu + u, (unsigned long long)bad);
        atomicMin(st + 3 * nu + u, (unsigned long long)first_bad);
    }
    if (miss) {
        atomicAdd(st + 2 * nu + u, 1ull);
        atomicMin(st + 4 * nu + u, (unsigned long long)first_miss);
    }
}

void launch_poseidon_chain(hipStream_t s, const PchTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    const uint32_t t = tab.t, R = tab.full + tab.partial;
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || t < 2 || t > POS_MAX_T || (tab.full & 1) || R == 0 ||
        R > POS_MAX_ROUNDS || tab.n_units == 0 || tab.n_units > PCH_MAX_UNITS || !tab.src || !tab.cst)
        return;
    uint64_t lanes = 0;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const PchUnit& U = tab.u[u];
        const bool path = U.mode == PCH_PATH, check = U.exp != PCH_NONE;
        auto row_ok = [](uint8_t v, bool escape) { return v < POLY_MAX_ROWS || (escape && v == PCH_NONE); };
        if ((!path && U.mode != PCH_SPONGE) || (path && t < 3) || U.period == 0) return;
        if (check ? (U.out || U.layout || U.exp >= POLY_MAX_ROWS) : (!U.out || (U.layout != PCH_TRACE && U.layout != PCH_FLAT))) return;
        if (U.layout == PCH_TRACE && U.period <= R) return;
        if (!row_ok(U.start, true) || (path ? U.pos >= POLY_MAX_ROWS : false)) return;
        if ((path || check) ? U.digest >= t : false) return;
        for (uint32_t i = 0; i < t; i++) {
            if (!row_ok(U.slot[i], !path || i < 2)) return;          // (POS_IMM is PCH_NONE; a path's siblings are rows)
            if (U.layout == PCH_FLAT && ((U.col[i] != PCH_NONE && U.col[i] >= 2 * t) ||
                                         (U.col[POS_MAX_T + i] != PCH_NONE && U.col[POS_MAX_T + i] >= 2 * t)))
                return;
        }
        const uint64_t l = n / U.period;
        lanes = l > lanes ? l : lanes;
    }
    if (!lanes) return;   // (every period above n: the zeroed columns are the result)
    const dim3 grid(nblk(lanes, 256), tab.n_units);
    const size_t smem = (size_t)(t * R + t * t + t) * 36;
    auto* sp = reinterpret_cast<unsigned long long*>(stats);
    switch (t) {
    case 2: k_fr_poseidon_chain<2><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 3: k_fr_poseidon_chain<3><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 4: k_fr_poseidon_chain<4><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 5: k_fr_poseidon_chain<5><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 6: k_fr_poseidon_chain<6><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 7: k_fr_poseidon_chain<7><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    default: k_fr_poseidon_chain<8><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    }
}
