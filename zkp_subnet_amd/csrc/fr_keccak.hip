// fr_keccak.hip -- Fr-side kernels, part 18: the Keccak-f[1600] permutation columns of kzg_rows_commit_keccak.  Every value is a
// 64-bit lane: a source cell is its CANONICAL INTEGER reduced to its low 64 bits (int_load of fr_u64.hip.h; a cell at or above
// 2^64 is counted), an output cell is the Montgomery form of a lane (int_store).  Source columns lie as evaluation vectors of T
// elements of 8 words, Montgomery, canonical.  FIPS 202 names: lane (x, y) of the state A has the flat index x + 5 y; a round is
// theta (the column parities C, the words D), rho (the rotation offsets r[x][y]), pi, chi and iota (the 24 round constants RC,
// constant memory, read with a uniform index).
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE kernel k_fr_keccak whose two unit forms branch on the
//   unit's mode, which is uniform over the workgroup.  No barrier anywhere: the 50 KB of LDS are 25 lanes of 64 bits PER LANE
//   of the device (word k of device lane v at lds[256 k + v]), a private array that may be indexed by a uniform variable
//   without leaving the registers' side for scratch.  The STATE itself never goes there to be permuted: its 25 lanes are 50
//   VGPRs, theta, rho, pi and chi are unrolled inside the round so that every index is a compile-time constant, and the 24
//   rounds are a real loop of that one body.  A rotation by a known amount is two v_alignbit_b32, the halves swapped at 32 or
//   more.
//     a ROW unit     one lane per row t' < n.  Each DISTINCT source cell of the row is loaded once (a real loop over the unit's
//                    list of distinct vectors: one int_load body) into the lane's LDS words; the 25 slots then pick their
//                    lane, or the slot's immediate, into registers.  The permuted state goes back to LDS, and a real loop over
//                    the unit's output columns stores lane out[c] (one int_store body) or, in a check, compares it with the
//                    expected cell.
//     a ROUNDS unit  one lane per MESSAGE.  The lane of block b reads its `start` cell; where b starts a message it walks
//                    forward block by block until the next start or the last block, the lanes of continuing blocks leave.
//                    Stores dominate here (up to 16 encoded cells per row), so a round's named cells are written as they are
//                    produced: after each of the five stages (the state, the running parities, D, theta and rho, pi) the 25
//                    values of the stage go to the lane's LDS words and one loop over the unit's columns stores the five rows
//                    of those that the stage serves; a stage that no column names is not staged.  The cells between and behind
//                    the blocks, and the cells where a column is undefined, were zeroed by the caller.  A single message that
//                    fills the column runs on ONE lane: a known limit (DESIGN.md has its measure).
//   Stores are int_store's two 16-byte vector stores of a whole cell.  Statistics: a lane that met an over-range cell, a
//   mismatch or the start of a message adds to the unit's words with plain atomics (such lanes are the exception, and the
//   compiler folds the adds of a wave into one).
// Bound: a ROW unit is 24 rounds of about 150 64-bit logic operations against 32 (distinct sources + outputs) B of traffic and
// one field product per cell moved; a ROUNDS unit is its stores: one product of radix 2^87 and 32 B per named cell.
#include <cstring>

#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

__constant__ uint64_t KEC_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// r[x][y] at x + 5 y
constexpr uint32_t KEC_ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// x rotated left by k < 64, k known where the call is unrolled: two v_alignbit_b32, the halves swapped first at k >= 32
KZG_DEV uint64_t kec_rotl(uint64_t x, uint32_t k) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (k >= 32) {
        const uint32_t t = lo;
        lo = hi;
        hi = t;
        k -= 32;
    }
    if (k == 0) return ((uint64_t)hi << 32) | lo;
    const uint32_t nl = __builtin_amdgcn_alignbit(lo, hi, 32 - k), nh = __builtin_amdgcn_alignbit(hi, lo, 32 - k);
    return ((uint64_t)nh << 32) | nl;
}

// the lane's private 64-bit value k: words 2 k and 2 k + 1 of its LDS column
KZG_DEV void kec_put(uint32_t* my, uint32_t k, uint64_t v) {
    my[256 * (2 * k)] = (uint32_t)v;
    my[256 * (2 * k + 1)] = (uint32_t)(v >> 32);
}
KZG_DEV uint64_t kec_get(const uint32_t* my, uint32_t k) { return ((uint64_t)my[256 * (2 * k + 1)] << 32) | my[256 * (2 * k)]; }

// c flagged cells of a lane, the smallest of them at `row`
KZG_DEV void kec_stat(uint32_t c, uint64_t row, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first) {
    if (!c) return;
    atomicAdd(cnt, (unsigned long long)c);
    atomicMin(first, (unsigned long long)row);
}

// theta up to D from the state A: C[x] the parity of column x, D[x] = C[x - 1] ^ rotl(C[x + 1], 1)
KZG_DEV void kec_theta(const uint64_t (&A)[25], uint64_t (&D)[5]) {
    uint64_t C[5];
#pragma unroll
    for (int x = 0; x < 5; x++) C[x] = A[x] ^ A[x + 5] ^ A[x + 10] ^ A[x + 15] ^ A[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) D[x] = C[(x + 4) % 5] ^ kec_rotl(C[(x + 1) % 5], 1);
}
// A <- the lanes after theta and rho at their source positions: rotl(A[x][y] ^ D[x], r[x][y])
KZG_DEV void kec_rho(uint64_t (&A)[25], const uint64_t (&D)[5]) {
#pragma unroll
    for (int i = 0; i < 25; i++) A[i] = kec_rotl(A[i] ^ D[i % 5], KEC_ROT[i]);
}
// B <- pi of the lanes t: B[y'][(2 x' + 3 y') mod 5] = t[x'][y']
KZG_DEV void kec_pi(uint64_t (&B)[25], const uint64_t (&t)[25]) {
#pragma unroll
    for (int x = 0; x < 5; x++)
#pragma unroll
        for (int y = 0; y < 5; y++) B[y + 5 * ((2 * x + 3 * y) % 5)] = t[x + 5 * y];
}
// A <- chi of B, then iota with the constant rc
KZG_DEV void kec_chi(uint64_t (&A)[25], const uint64_t (&B)[25], uint64_t rc) {
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) A[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
    A[0] ^= rc;
}
// Keccak-f[1600]: a real loop over the rounds of one unrolled body
KZG_DEV void kec_permute(uint64_t (&A)[25]) {
#pragma unroll 1
    for (uint32_t r = 0; r < 24; r++) {
        uint64_t D[5], B[25];
        kec_theta(A, D);
        kec_rho(A, D);
        kec_pi(B, A);
        kec_chi(A, B, KEC_RC[r]);
    }
}

// one permutation per row: lane `row` < n of a ROW unit
KZG_DEV void kec_row_unit(const KecTab& tab, const KecUnit& U, uint64_t T, uint64_t row, uint32_t* my, unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    uint32_t over = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < U.n_ld; k++) {
        bool o;
        kec_put(my, k, int_load(tab.src + 8 * ((uint64_t)U.ld[k] * T + row), &o));
        over += o;
    }
    uint64_t A[25];
#pragma unroll
    for (int j = 0; j < 25; j++) {
        const uint32_t sl = U.slot[j];
        const uint64_t w = kec_get(my, sl == KEC_IMM ? 0u : sl);
        A[j] = sl == KEC_IMM ? U.imm[j] : w;
    }
    kec_permute(A);
#pragma unroll
    for (int j = 0; j < 25; j++) kec_put(my, j, A[j]);
    uint32_t differs = 0;
#pragma unroll 1
    for (uint32_t col = 0; col < U.n_out; col++) {
        const uint64_t w = kec_get(my, U.col[col]);
        if (U.out) {
            int_store(U.out + 8 * ((uint64_t)col * T + row), w);
        } else {
            bool o;
            const uint64_t x = int_load(tab.src + 8 * ((uint64_t)U.exp[col] * T + row), &o);
            differs |= o || x != w;
        }
    }
    kec_stat(over, row, st + u, st + 3 * nu + u);
    kec_stat(differs, row, st + nu + u, st + 4 * nu + u);
}

// the five rows row0 .. row0 + 4 of the named columns of one kind (a, p, d, t, b: the column id is 5 kind + x) from the lane's 25
// staged values, value (x, y) at x + 5 y
KZG_DEV void kec_emit(const KecUnit& U, const uint32_t* my, uint64_t T, uint64_t row0, uint32_t kind) {
#pragma unroll 1
    for (uint32_t c = 0; c < U.n_out; c++) {
        const uint32_t id = U.col[c];
        if (id / 5 != kind) continue;
        const uint32_t x = id % 5;
#pragma unroll 1
        for (uint32_t y = 0; y < 5; y++) int_store(U.out + 8 * ((uint64_t)c * T + row0 + y), kec_get(my, x + 5 * y));
    }
}

// one message per lane: lane b0 < nb of a ROUNDS unit, nb = floor(n / P) blocks
KZG_DEV void kec_rounds_unit(const KecTab& tab, const KecUnit& U, uint64_t T, uint64_t nb, uint64_t b0, uint32_t* my,
                             unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const uint64_t P = U.period;
    const uint32_t* start = U.ld[5] == KEC_IMM ? nullptr : tab.src + 8 * (uint64_t)U.ld[5] * T;
    uint32_t over = 0;
    uint64_t first = ~0ull;
    bool begins = b0 == 0 || !start;
    if (start) {   // (the lane of a block is the one that counts the block's start cell)
        bool o;
        begins |= int_load(start + 8 * b0 * P, &o) != 0;
        if (o) {
            over = 1;
            first = b0 * P;
        }
    }
    if (begins) {
        atomicAdd(st + 2 * nu + u, 1ull);
        uint32_t kinds = 0;   // the stages some column names
        for (uint32_t c = 0; c < U.n_out; c++) kinds |= 1u << (U.col[c] / 5);
        uint64_t A[25];
#pragma unroll
        for (int i = 0; i < 25; i++) A[i] = 0;
        for (uint64_t b = b0;;) {
            const uint64_t base = b * P;
            // absorb: lane i = x + 5 y < rate takes the cell of msg[x] at block row y.  One cell may serve several lanes (a
            // repeated msg row, or the start column at y = 0): nocount marks the lanes whose cell another reader counts
#pragma unroll 1
            for (uint32_t i = 0; i < U.rate; i++) {
                const uint32_t x = i % 5, y = i / 5;
                bool o;
                kec_put(my, i, int_load(tab.src + 8 * ((uint64_t)U.ld[x] * T + base + y), &o));
                if (o && !(U.nocount >> i & 1)) {
                    over++;
                    first = first < base + y ? first : base + y;
                }
            }
#pragma unroll
            for (int i = 0; i < 24; i++) {
                const uint64_t m = kec_get(my, i);
                A[i] ^= (uint32_t)i < U.rate ? m : 0;
            }
#pragma unroll 1
            for (uint32_t r = 0; r < 24; r++) {
                const uint64_t row0 = base + 5 * r;
                if (kinds & 1) {
#pragma unroll
                    for (int i = 0; i < 25; i++) kec_put(my, i, A[i]);
                    kec_emit(U, my, T, row0, 0);
                }
                if (kinds & 2) {
#pragma unroll
                    for (int x = 0; x < 5; x++) {
                        uint64_t p = 0;
#pragma unroll
                        for (int y = 0; y < 5; y++) {
                            p ^= A[x + 5 * y];
                            kec_put(my, x + 5 * y, p);
                        }
                    }
                    kec_emit(U, my, T, row0, 1);
                }
                uint64_t D[5], B[25];
                kec_theta(A, D);
                if (kinds & 4) {
#pragma unroll
                    for (int i = 0; i < 25; i++) kec_put(my, i, D[i % 5]);
                    kec_emit(U, my, T, row0, 2);
                }
                kec_rho(A, D);
                if (kinds & 8) {
#pragma unroll
                    for (int i = 0; i < 25; i++) kec_put(my, i, A[i]);
                    kec_emit(U, my, T, row0, 3);
                }
                kec_pi(B, A);
                if (kinds & 16) {
#pragma unroll
                    for (int i = 0; i < 25; i++) kec_put(my, i, B[i]);
                    kec_emit(U, my, T, row0, 4);
                }
                kec_chi(A, B, KEC_RC[r]);
            }
            if (kinds & 1) {   // rows 120 .. 124: the outgoing state, in the a columns only
#pragma unroll
                for (int i = 0; i < 25; i++) kec_put(my, i, A[i]);
                kec_emit(U, my, T, base + 120, 0);
            }
            if (++b >= nb || !start) break;
            bool o;   // (read again by the lane of block b, which counts it)
            if (int_load(start + 8 * b * P, &o) != 0) break;
        }
    }
    kec_stat(over, first, st + u, st + 3 * nu + u);
}

// T a power of two, n <= T; every ld, slot, col and exp of a unit either its escape value or inside its range (the launcher's
// and its caller's checks).  Lanes past the unit's last one read nothing and store nothing
__global__ void __launch_bounds__(256) k_fr_keccak(const KecTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    __shared__ uint32_t lds[KEC_LANE_WORDS * 256];
    const KecUnit& U = tab.u[blockIdx.y];
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* my = lds + threadIdx.x;
    if (U.mode == KEC_ROUNDS) {
        const uint64_t nb = n / U.period;
        if (v < nb) kec_rounds_unit(tab, U, T, nb, v, my, st);
    } else if (v < n) {
        kec_row_unit(tab, U, T, v, my, st);
    }
}

void launch_keccak(hipStream_t s, const KecTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || tab.n_units == 0 || tab.n_units > KEC_MAX_UNITS || !tab.src)
        return;
    uint64_t lanes = 0;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const KecUnit& U = tab.u[u];
        const bool rounds = U.mode == KEC_ROUNDS;
        if (!rounds && U.mode != KEC_ROW) return;
        if (U.n_out == 0 || U.n_out > KEC_MAX_OUT) return;
        for (uint32_t c = 0; c < U.n_out; c++) {
            if (U.col[c] >= KEC_N_COLS) return;
            if (!rounds && !U.out && U.exp[c] >= POLY_MAX_ROWS) return;
        }
        if (rounds) {
            if (U.period < KEC_MIN_PERIOD || !U.out || U.rate == 0 || U.rate > 24 || (U.ld[5] != KEC_IMM && U.ld[5] >= POLY_MAX_ROWS))
                return;
            for (uint32_t x = 0; x < 5; x++)
                if (U.ld[x] >= POLY_MAX_ROWS) return;
        } else {
            if (U.n_ld > POLY_MAX_ROWS) return;
            for (uint32_t k = 0; k < U.n_ld; k++)
                if (U.ld[k] >= POLY_MAX_ROWS) return;
            for (uint32_t j = 0; j < 25; j++)
                if (U.slot[j] != KEC_IMM && U.slot[j] >= U.n_ld) return;
        }
        const uint64_t l = rounds ? n / U.period : n;
        lanes = l > lanes ? l : lanes;
    }
    if (!lanes) return;   // (only ROUNDS units, each with a period above n: their zeroed columns are the result)
    k_fr_keccak<<<dim3(nblk(lanes, 256), tab.n_units), 256, 0, s>>>(tab, T, n, reinterpret_cast<unsigned long long*>(stats));
}
