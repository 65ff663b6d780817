// fr_poseidon.hip -- Fr-side kernels, part 16: the Poseidon permutation columns of kzg_rows_commit_poseidon.  The plain Hades
// schedule over Fr with the S-box x^5: for each round rho < R = R_F + R_P: s_i += rc[rho t + i]; s_i <- s_i^5 for every i in a
// full round (rho < R_F / 2 or rho >= R_F / 2 + R_P), for i = 0 only in a partial one; s <- M s.  Source columns lie as
// evaluation vectors of T elements of 8 words, Montgomery, CANONICAL (the forward transform ends in fr9_reduce).
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE body k_fr_poseidon<t> for the three unit forms: the state
//   is t fr9_t in registers, indexed by constants only, and the round loop's trip counts are uniform.  The S-boxes of a round
//   and the rows of M are REAL loops (#pragma unroll 1) whose element is picked and put back by uniform selects: unrolled, the
//   compiler hoisted the t t entries of M out of the round loop and interleaved the t S-boxes, 304 .. 784 B of scratch per lane
//   from t = 4 on; as loops no instantiation has scratch (t = 2 .. 4: 110 / 152 / 212 VGPRs; t = 5 .. 8: 256 and 18 .. 222 AGPRs),
//   and a round's code is one S-box and one row of M.
//     a ROW unit     one lane per row t' < n: the permutation, then one store per output column;
//     a check        the same lane compares instead of storing; rows that differ are counted through derive_count, the
//                    smallest one found through expr_first;
//     a ROUNDS unit  one lane per block of P rows, floor(n / P) lanes: a store of the t state elements before every round and
//                    behind the last, R + 1 rows of the block; the rows between the blocks were zeroed by the caller.
//   The constants -- t R round constants, t t matrix entries, the unit's t immediates -- come from a device buffer as 8 words
//   of a canonical integer each (up to 8 144 + 64 + 8 scalars of 9 limbs do not fit a 4 KB kernel argument) and are converted
//   to Montgomery form into LDS once per workgroup, (t R + t t + t) x 36 bytes of dynamic LDS, at most 44064.
//   Operand classes (fr29.hip.h).  The state is canonical at the head of every round (a loaded cell, an immediate from LDS, or
//   fr9_reduce's output).  u = s + rc: both canonical, below 2 r with limbs below 2^30.  Under an S-box u is normalised (a
//   legal SECOND operand, and u u < 4 r^2 is far inside 2^261 r = 70 r^2); u^2 and u^4 are products' outputs (N class), legal
//   on both sides; u^5 = u^4 u.  Outside the S-box u stays lazy: a legal FIRST operand.  The matrix row: x_j M_ij with x_j the
//   first operand (N or lazy below 2 r) and M_ij canonical from LDS the second; every product is below 2 r with limbs 0 .. 7
//   below 2^29, and the sum is renormalised after every third term, so that its limbs stay below 2^31 and its value below 16 r
//   for t = 8 -- inside the 64 r that fr9_reduce takes, which closes with fr9_canon.  Every stored cell is canonical, every
//   store is a vector store (fr9_store: two 16-byte stores).
// Bound: a permutation is R_F (3 t + t^2) + R_P (3 + t^2) field products per lane -- 828 at t = 3, (8, 57) -- against 32 t B read
// and 32 n_out B written (ROUNDS: 32 t (R + 1) B written): the multiplier by three orders of magnitude.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

KZG_DEV void pos_lds(fr9_t& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
}

// T a power of two, n <= T; every slot, col and exp of the unit either its escape value or the index of a vector below src /
// out (the launcher's and its caller's checks).  Workgroups past the unit's last lane leave at once (before any barrier);
// lanes past it inside the last workgroup read nothing and store nothing; they still walk the two reductions.
template <int TW>
__global__ void __launch_bounds__(256) k_fr_poseidon(const PosTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    extern __shared__ uint32_t lds[];   // [t R] rc, [t t] M, [t] the unit's immediates: 9 limbs each
    const PosUnit& U = tab.u[blockIdx.y];
    const uint32_t R = tab.full + tab.partial, half = tab.full / 2, nrc = TW * R, nc = nrc + TW * TW + TW;
    const bool rounds = U.mode == POS_ROUNDS;
    const uint64_t lanes = rounds ? n / U.period : n;
    if ((uint64_t)blockIdx.x * blockDim.x >= lanes) return;
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
    bool differs = false;
    if (v < lanes) {
        const uint64_t row = rounds ? v * U.period : v;
        fr9_t s[TW];
#pragma unroll
        for (int i = 0; i < TW; i++) {
            if (U.slot[i] == POS_IMM) pos_lds(s[i], imm + 9 * i);
            else fr9_load(s[i], tab.src + 8 * (U.slot[i] * T + row));
            if (rounds) fr9_store(U.out + 8 * (i * T + row), s[i]);
        }
        for (uint32_t rho = 0; rho < R; rho++) {
            const bool full = rho < half || rho >= half + tab.partial;
            fr9_t x[TW];
#pragma unroll
            for (int i = 0; i < TW; i++) {
                fr9_t c;
                pos_lds(c, lds + 9 * (rho * TW + i));
                fr9_add(x[i], s[i], c);
            }
            const uint32_t n_sbox = full ? TW : 1;
#pragma unroll 1
            for (uint32_t i = 0; i < n_sbox; i++) {   // (a real loop again: one S-box in flight, x_i picked and put back by selects)
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
                pos_lds(m, mrow);
                fr9_mul(acc, x[0], m);
#pragma unroll
                for (int j = 1; j < TW; j++) {
                    pos_lds(m, mrow + 9 * j);
                    fr9_mul(p, x[j], m);
                    fr9_add(acc, acc, p);
                    if (j % 3 == 2 && j + 1 < TW) fr9_norm(acc, acc);
                }
                fr9_reduce(acc, acc);
#pragma unroll
                for (int k = 0; k < TW; k++)
                    if (k == (int)i) s[k] = acc;      // (i is uniform: a select per limb, the state stays in registers)
                if (rounds) fr9_store(U.out + 8 * (i * T + row + rho + 1), acc);
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

uint32_t poseidon_cst_words(uint32_t t, uint32_t rounds, uint32_t n_units) { return 8 * (t * rounds + t * t + t * n_units); }

void launch_poseidon(hipStream_t s, const PosTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    const uint32_t t = tab.t, R = tab.full + tab.partial;
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || t < 2 || t > POS_MAX_T || (tab.full & 1) || R == 0 ||
        R > POS_MAX_ROUNDS || tab.n_units == 0 || tab.n_units > POS_MAX_UNITS || !tab.src || !tab.cst)
        return;
    uint64_t lanes = 0;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const PosUnit& U = tab.u[u];
        const bool rounds = U.mode == POS_ROUNDS;
        if ((!rounds && U.mode != POS_ROW) || (rounds && (U.period <= R || !U.out))) return;
        for (uint32_t i = 0; i < t; i++) {
            if (U.slot[i] != POS_IMM && U.slot[i] >= POLY_MAX_ROWS) return;
            if (!rounds && U.col[i] != POS_NO_COL && (U.col[i] >= t || (!U.out && U.exp[U.col[i]] >= POLY_MAX_ROWS))) return;
        }
        const uint64_t l = rounds ? n / U.period : n;
        lanes = l > lanes ? l : lanes;
    }
    if (!lanes) return;   // (only ROUNDS units, each with a period above n: their zeroed columns are the result)
    const dim3 grid(nblk(lanes, 256), tab.n_units);
    const size_t smem = (size_t)(t * R + t * t + t) * 36;
    auto* sp = reinterpret_cast<unsigned long long*>(stats);
    switch (t) {
    case 2: k_fr_poseidon<2><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 3: k_fr_poseidon<3><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 4: k_fr_poseidon<4><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 5: k_fr_poseidon<5><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 6: k_fr_poseidon<6><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    case 7: k_fr_poseidon<7><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    default: k_fr_poseidon<8><<<grid, 256, smem, s>>>(tab, T, n, sp); break;
    }
}
