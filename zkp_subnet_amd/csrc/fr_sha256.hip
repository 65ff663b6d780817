// fr_sha256.hip -- Fr-side kernels, part 17: the SHA-256 compression columns of kzg_rows_commit_sha256.  Every value is a
// 32-bit word: a source cell is its CANONICAL INTEGER reduced to its low 32 bits (int_load of fr_u64.hip.h; a cell at or above
// 2^32 is counted), an output cell is the Montgomery form of a word (int_store).  Source columns lie as evaluation vectors of T
// elements of 8 words, Montgomery, canonical.  FIPS 180-4 names: Ch, Maj, the big Sigma0 / Sigma1 of a round, the small sigma0 /
// sigma1 of the schedule, the 64 constants K (constant memory, read with a uniform index), the chaining value H.
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE kernel k_fr_sha256 whose two unit forms branch on the
//   unit's mode, which is uniform over the workgroup.  No barrier anywhere: the 36 KB of LDS are 36 words PER LANE (word k of
//   lane v at lds[256 k + v]), a lane-private array that may be indexed by a uniform variable without leaving the registers'
//   side for scratch.
//     a ROW unit     one lane per row t' < n.  Each DISTINCT source cell of the row is loaded once (a real loop over the unit's
//                    list of distinct vectors: one int_load body) into the lane's LDS words; the 8 + 16 slots then pick their
//                    word, or the slot's immediate, into registers.  The 64 rounds are fully unrolled: the schedule is a
//                    16-word rolling window and the eight working variables rotate by renaming, both indexed by compile-time
//                    constants only, so that they stay in VGPRs; every rotation is one v_alignbit_b32.  The new chaining value
//                    goes back to LDS, and a real loop over the unit's output columns stores word out[c] (one int_store
//                    body) or, in a check, compares it with the expected cell.
//     a ROUNDS unit  one lane per MESSAGE.  The lane of block b reads its `start` cell; where b starts a message it walks
//                    forward block by block until the next start or the last block, the lanes of continuing blocks leave.
//                    Stores dominate here (up to 12 encoded cells per row), so the round is a REAL loop of one body: the
//                    window, the chaining value and the twelve values of the row live in the lane's LDS words, and one loop
//                    over the unit's columns stores those that are named and defined on the row.  The cells between and
//                    behind the blocks, and the cells where a column is undefined, were zeroed by the caller.  A single
//                    message that fills the column runs on ONE lane: a known limit (DESIGN.md has its measure).
//   Stores are int_store's two 16-byte vector stores of a whole cell.  Statistics: a lane that met an over-range cell, a
//   mismatch or the start of a message adds to the unit's words with plain atomics (such lanes are the exception, and the
//   compiler folds the adds of a wave into one).
// Bound: a ROW unit is 64 rounds of about 40 integer instructions against 32 (distinct sources + outputs) B of traffic and one
// field product per cell moved; a ROUNDS unit is its stores: one product of radix 2^87 and 32 B per named cell.
#include <cstring>

#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

__constant__ uint32_t SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
    0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
    0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
    0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

KZG_DEV uint32_t sha_rotr(uint32_t x, uint32_t k) { return __builtin_amdgcn_alignbit(x, x, k); }   // (one v_alignbit_b32)
KZG_DEV uint32_t sha_sig0(uint32_t x) { return sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3); }
KZG_DEV uint32_t sha_sig1(uint32_t x) { return sha_rotr(x, 17) ^ sha_rotr(x, 19) ^ (x >> 10); }
KZG_DEV uint32_t sha_sum0(uint32_t x) { return sha_rotr(x, 2) ^ sha_rotr(x, 13) ^ sha_rotr(x, 22); }
KZG_DEV uint32_t sha_sum1(uint32_t x) { return sha_rotr(x, 6) ^ sha_rotr(x, 11) ^ sha_rotr(x, 25); }
KZG_DEV uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return (e & f) ^ (~e & g); }
KZG_DEV uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) ^ (a & c) ^ (b & c); }

// the low 32 bits of the cell at p; *over <- whether the cell's integer is at or above 2^32
KZG_DEV uint32_t sha_load(const uint32_t* p, bool* over) {
    bool high;
    const uint64_t v = int_load(p, &high);
    *over = high || (v >> 32) != 0;
    return (uint32_t)v;
}
// c flagged cells of a lane, the smallest of them at `row`
KZG_DEV void sha_stat(uint32_t c, uint64_t row, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first) {
    if (!c) return;
    atomicAdd(cnt, (unsigned long long)c);
    atomicMin(first, (unsigned long long)row);
}

// one compression per row: lane `row` < n of a ROW unit
KZG_DEV void sha_row_unit(const ShaTab& tab, const ShaUnit& U, uint64_t T, uint64_t row, uint32_t* my, unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    uint32_t over = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < U.n_ld; k++) {
        bool o;
        my[256 * k] = sha_load(tab.src + 8 * ((uint64_t)U.ld[k] * T + row), &o);
        over += o;
    }
    uint32_t s[8], m[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t sl = U.slot[j], w = my[256 * (sl == SHA_IMM ? 0u : sl)];
        s[j] = sl == SHA_IMM ? U.imm[j] : w;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t sl = U.slot[8 + j], w = my[256 * (sl == SHA_IMM ? 0u : sl)];
        m[j] = sl == SHA_IMM ? U.imm[8 + j] : w;
    }
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) m[t & 15] += sha_sig1(m[(t - 2) & 15]) + m[(t - 7) & 15] + sha_sig0(m[(t - 15) & 15]);
        const uint32_t t1 = h + sha_sum1(e) + sha_ch(e, f, g) + SHA_K[t] + m[t & 15], t2 = sha_sum0(a) + sha_maj(a, b, c);
        h = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    my[0] = s[0] + a;
    my[256] = s[1] + b;
    my[512] = s[2] + c;
    my[768] = s[3] + d;
    my[1024] = s[4] + e;
    my[1280] = s[5] + f;
    my[1536] = s[6] + g;
    my[1792] = s[7] + h;
    uint32_t differs = 0;
#pragma unroll 1
    for (uint32_t col = 0; col < U.n_out; col++) {
        const uint32_t w = my[256 * U.col[col]];
        if (U.out) {
            int_store(U.out + 8 * ((uint64_t)col * T + row), w);
        } else {
            bool o;
            const uint32_t x = sha_load(tab.src + 8 * ((uint64_t)U.exp[col] * T + row), &o);
            differs |= o || x != w;
        }
    }
    sha_stat(over, row, st + u, st + 3 * nu + u);
    sha_stat(differs, row, st + nu + u, st + 4 * nu + u);
}

// the named columns that are defined on a row (bits of `mask`, by column id) from the lane's twelve values V
KZG_DEV void sha_emit(const ShaUnit& U, const uint32_t* V, uint64_t T, uint64_t row, uint32_t mask) {
#pragma unroll 1
    for (uint32_t c = 0; c < U.n_out; c++) {
        const uint32_t id = U.col[c];
        if (mask >> id & 1) int_store(U.out + 8 * ((uint64_t)c * T + row), V[256 * id]);
    }
}

// one message per lane: lane b0 < nb of a ROUNDS unit, nb = floor(n / P) blocks
KZG_DEV void sha_rounds_unit(const ShaTab& tab, const ShaUnit& U, uint64_t T, uint64_t nb, uint64_t b0, uint32_t* my,
                             unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const uint64_t P = U.period;
    const uint32_t* msg = tab.src + 8 * (uint64_t)U.ld[0] * T;
    const uint32_t* start = U.ld[1] == SHA_IMM ? nullptr : tab.src + 8 * (uint64_t)U.ld[1] * T;
    uint32_t over = 0;
    uint64_t first = ~0ull;
    bool begins = b0 == 0 || !start;
    if (start) {   // (the lane of a block is the one that counts the block's start cell)
        bool o;
        begins |= sha_load(start + 8 * b0 * P, &o) != 0;
        if (o) {
            over = 1;
            first = b0 * P;
        }
    }
    if (begins) {
        atomicAdd(st + 2 * nu + u, 1ull);
        uint32_t *W = my, *H = my + 16 * 256, *V = my + 24 * 256;   // the window (then the last working variables), H, the row
        constexpr uint32_t AE = 1u << SHA_COL_A | 1u << SHA_COL_E, FF = AE | 1u << SHA_COL_CA | 1u << SHA_COL_CE,
                           HEAD = 0xfffu & ~(1u << SHA_COL_CW | 1u << SHA_COL_SIG0 | 1u << SHA_COL_SIG1);
#pragma unroll
        for (int i = 0; i < 8; i++) H[256 * i] = U.imm[i];
        for (uint64_t b = b0;;) {
            const uint64_t base = b * P;
#pragma unroll 1
            for (uint32_t j = 0; j < 4; j++) {
                V[256 * SHA_COL_A] = H[256 * (3 - j)];
                V[256 * SHA_COL_E] = H[256 * (7 - j)];
                sha_emit(U, V, T, base + j, AE);
            }
            uint32_t a = H[0], bb = H[256], c = H[512], d = H[768], e = H[1024], f = H[1280], g = H[1536], h = H[1792];
#pragma unroll 1
            for (uint32_t t = 0; t < 64; t++) {
                const uint64_t row = base + 4 + t;
                uint32_t w, s0 = 0, s1 = 0, cw = 0;
                if (t < 16) {
                    bool o;
                    w = sha_load(msg + 8 * row, &o);
                    if (o) {
                        over++;
                        first = first < row ? first : row;
                    }
                } else {
                    s1 = sha_sig1(W[256 * ((t - 2) & 15)]);
                    s0 = sha_sig0(W[256 * ((t - 15) & 15)]);
                    const uint64_t sum = (uint64_t)s1 + W[256 * ((t - 7) & 15)] + s0 + W[256 * (t & 15)];
                    w = (uint32_t)sum;
                    cw = (uint32_t)(sum >> 32);
                }
                W[256 * (t & 15)] = w;
                const uint32_t S1 = sha_sum1(e), ch = sha_ch(e, f, g), S0 = sha_sum0(a), mj = sha_maj(a, bb, c);
                const uint64_t t1 = (uint64_t)h + S1 + ch + SHA_K[t] + w, sa = t1 + S0 + mj, se = t1 + d;
                V[256 * SHA_COL_W] = w;
                V[256 * SHA_COL_A] = (uint32_t)sa;
                V[256 * SHA_COL_E] = (uint32_t)se;
                V[256 * SHA_COL_CW] = cw;
                V[256 * SHA_COL_CA] = (uint32_t)(sa >> 32);
                V[256 * SHA_COL_CE] = (uint32_t)(se >> 32);
                V[256 * SHA_COL_SIG0] = s0;
                V[256 * SHA_COL_SIG1] = s1;
                V[256 * SHA_COL_SUM0] = S0;
                V[256 * SHA_COL_MAJ] = mj;
                V[256 * SHA_COL_SUM1] = S1;
                V[256 * SHA_COL_CH] = ch;
                sha_emit(U, V, T, row, t < 16 ? HEAD : 0xfffu);
                h = g;
                g = f;
                f = e;
                e = (uint32_t)se;
                d = c;
                c = bb;
                bb = a;
                a = (uint32_t)sa;
            }
            W[0] = a;
            W[256] = bb;
            W[512] = c;
            W[768] = d;
            W[1024] = e;
            W[1280] = f;
            W[1536] = g;
            W[1792] = h;
#pragma unroll 1
            for (uint32_t j = 0; j < 4; j++) {   // row 68 + j: A[j] + A[64 + j] is H[3 - j] + (d, c, b, a)[j], and so for E
                const uint64_t fa = (uint64_t)H[256 * (3 - j)] + W[256 * (3 - j)], fe = (uint64_t)H[256 * (7 - j)] + W[256 * (7 - j)];
                H[256 * (3 - j)] = (uint32_t)fa;
                H[256 * (7 - j)] = (uint32_t)fe;
                V[256 * SHA_COL_A] = (uint32_t)fa;
                V[256 * SHA_COL_E] = (uint32_t)fe;
                V[256 * SHA_COL_CA] = (uint32_t)(fa >> 32);
                V[256 * SHA_COL_CE] = (uint32_t)(fe >> 32);
                sha_emit(U, V, T, base + 68 + j, FF);
            }
            if (++b >= nb || !start) break;
            bool o;   // (read again by the lane of block b, which counts it)
            if (sha_load(start + 8 * b * P, &o) != 0) break;
        }
    }
    sha_stat(over, first, st + u, st + 3 * nu + u);
}

// T a power of two, n <= T; every ld, slot, col and exp of a unit either its escape value or inside its range (the launcher's
// and its caller's checks).  Lanes past the unit's last one read nothing and store nothing
__global__ void __launch_bounds__(256) k_fr_sha256(const ShaTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    __shared__ uint32_t lds[SHA_LANE_WORDS * 256];
    const ShaUnit& U = tab.u[blockIdx.y];
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* my = lds + threadIdx.x;
    if (U.mode == SHA_ROUNDS) {
        const uint64_t nb = n / U.period;
        if (v < nb) sha_rounds_unit(tab, U, T, nb, v, my, st);
    } else if (v < n) {
        sha_row_unit(tab, U, T, v, my, st);
    }
}

void launch_sha256(hipStream_t s, const ShaTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || tab.n_units == 0 || tab.n_units > SHA_MAX_UNITS || !tab.src)
        return;
    uint64_t lanes = 0;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const ShaUnit& U = tab.u[u];
        const bool rounds = U.mode == SHA_ROUNDS;
        if (!rounds && U.mode != SHA_ROW) return;
        if (U.n_out == 0 || U.n_out > (rounds ? SHA_N_COLS : 8u)) return;
        for (uint32_t c = 0; c < U.n_out; c++) {
            if (U.col[c] >= (rounds ? SHA_N_COLS : 8u)) return;
            if (!rounds && !U.out && U.exp[c] >= POLY_MAX_ROWS) return;
        }
        if (rounds) {
            if (U.period < SHA_MIN_PERIOD || !U.out || U.ld[0] >= POLY_MAX_ROWS || (U.ld[1] != SHA_IMM && U.ld[1] >= POLY_MAX_ROWS))
                return;
        } else {
            if (U.n_ld > POLY_MAX_ROWS) return;
            for (uint32_t k = 0; k < U.n_ld; k++)
                if (U.ld[k] >= POLY_MAX_ROWS) return;
            for (uint32_t j = 0; j < 24; j++)
                if (U.slot[j] != SHA_IMM && U.slot[j] >= U.n_ld) return;
        }
        const uint64_t l = rounds ? n / U.period : n;
        lanes = l > lanes ? l : lanes;
    }
    if (!lanes) return;   // (only ROUNDS units, each with a period above n: their zeroed columns are the result)
    k_fr_sha256<<<dim3(nblk(lanes, 256), tab.n_units), 256, 0, s>>>(tab, T, n, reinterpret_cast<unsigned long long*>(stats));
}
