// fr_wide.hip -- Fr-side kernels, part 15: the multi-limb integer columns of kzg_rows_commit_wide.  A WIDE VALUE is L consecutive
// source columns, limb l in column first + l, little-endian; every limb cell is read as its canonical integer and reduced to
// its low b bits (1 <= b <= 64, 1 <= L <= 8, W = b L <= 512).  The kinds: add with its carry, sub with its borrow, the 2 W-bit
// product, quotient and remainder, r = (a b + d) mod m with its quotient, and the carry columns of that identity limb by limb.
// A source column lies as an evaluation vector (T elements of 8 words, Montgomery, CANONICAL); rows [0, n) are read.
//   ONE launch per call: grid (blocks over n, n_ops), 256 lanes per workgroup, one lane per row of one op.  The op table rides in
//   the kernel argument (200 B per op), so kind, b, L, count and the vector slots are scalar loads and every branch on them is
//   uniform over the workgroup.  The kernel is instantiated on N = 4, 8 or 16, the number of 32-bit words that holds the widest
//   W of the call.  A wide value is a VECTOR of N words (wv<N>), never an array: a vector is no object in memory, every index
//   into it is a compile-time constant after unrolling, and so nothing is addressed dynamically.  (As arrays the same code kept
//   its values in private memory: the optimiser merged neighbouring words into wider accesses before it split the arrays.)
//   PACKING: a wide operand is built from its top limb down, X <- (X << b) | limb, so the limb loop may roll (one int_load body
//   per operand) while the word indices stay constant; the outputs leave the same way, limb <- X mod 2^b, X <- X >> b, with one
//   int_store body.  A shift by b is two or one word moves (b = 64, b >= 32) and a funnel shift by b mod 32 through a 64-bit
//   intermediate, so the counts 0, 32 and 64 meet no undefined shift.  An operand b whose limbs are the rows of a is not loaded.
//   DIVISION (divmod, mulmod, and c mod m for KZG_WIDE_NEG_C where c > m): Knuth's algorithm D on 32-bit digits, a 2N-word
//   dividend by an N-word divisor.  The divisor is shifted left until bit 32 N - 1 is set -- whole words through a barrel of
//   selects (1, 2, 4, 8 words), the rest through the funnel shift, a shift of 0 included -- and the dividend with it into 3 N
//   words, so every divisor has N digits.  The 2 N digit steps ROLL over a fixed window: a step works on the top N + 1 words,
//   then the dividend moves up one word and the digit enters the quotient from below, so the indices are constants without
//   unrolling 2 N steps of N products (unrolled, the N = 16 body passed the unroll budget and fell into private memory).  A
//   step estimates qhat from the two top words with a precomputed reciprocal of the divisor's top word (Moeller and Granlund's
//   2-by-1 step, ONE 64-bit division per lane), corrects it at most twice against the divisor's second word, subtracts qhat V
//   and adds V back where that borrowed.  A zero divisor is replaced by 1 before, and its outputs selected after.  ONE body of
//   the division is compiled per instantiation: the two uses of a row (c mod m, then the kind's own) are passes of a rolled loop.
//   The carry kind works on the limbs themselves: s_k in a signed 128-bit accumulator (b <= 56: eight products below 2^112);
//   the carries wait in registers and leave through one encoder body.
//   A row with a limb at or above 2^b is counted ONCE through derive_count, the first such row through expr_first; a quotient at
//   or above 2^W (mulmod) or an inexact row (carry) the same way in a second pair.  Lanes t >= n read nothing and store nothing;
//   they still walk the reductions.
//   Registers (gfx950, the compiler's resource remarks): N = 4: 184 VGPRs, no scratch, 2 waves per SIMD; N = 8: 254 VGPRs, no
//   scratch, 1 wave; N = 16: 256 VGPRs and 1004 B of scratch per lane (spills of the 48 + 32 + 16-word division state beside
//   the operands), 1 wave.  DESIGN.md has the table.
// Bound: compute.  Per row of a 512-bit mulmod: 256 products of the schoolbook, 32 digit steps of 16 multiply-subtracts, 16
// decoded and 16 encoded cells.
#include <cstring>

#include "../../include/kzg_mi355x.h"   // the KZG_WIDE_* kinds and flags
#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// ---- words: every count is a compile-time constant, every shift count below 32
// the high word of (hi : lo) << s, 0 <= s < 32
KZG_DEV uint32_t funnel_l(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)(((((uint64_t)hi << 32) | lo) << s) >> 32); }
// the low word of (hi : lo) >> s, 0 <= s < 32
KZG_DEV uint32_t funnel_r(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> s); }

// K words as ONE value: a vector is never an object in memory, so its elements stay in registers whatever the optimiser makes
// of the loops around it; every index is a compile-time constant once the loops are unrolled
template <int K>
using wv = uint32_t __attribute__((ext_vector_type(K)));

template <int K>
KZG_DEV void w_zero(wv<K>& x) {
#pragma unroll
    for (int i = 0; i < K; i++) x[i] = 0;
}
// x <- x << 32 where `on` (a select per word: `on` may differ from lane to lane)
template <int K, int D>
KZG_DEV void w_up(wv<K>& x, bool on) {
#pragma unroll
    for (int i = K - 1; i >= 0; i--) x[i] = on ? (i >= D ? x[i - (i >= D ? D : 0)] : 0u) : x[i];
}
template <int K, int D>
KZG_DEV void w_down(wv<K>& x, bool on) {
#pragma unroll
    for (int i = 0; i < K; i++) x[i] = on ? (i + D < K ? x[i + (i + D < K ? D : 0)] : 0u) : x[i];
}
template <int K>
KZG_DEV void w_shl_bits(wv<K>& x, uint32_t s) {   // s < 32
#pragma unroll
    for (int i = K - 1; i >= 1; i--) x[i] = funnel_l(x[i], x[i - 1], s);
    x[0] = funnel_l(x[0], 0u, s);
}
template <int K>
KZG_DEV void w_shr_bits(wv<K>& x, uint32_t s) {   // s < 32
#pragma unroll
    for (int i = 0; i < K - 1; i++) x[i] = funnel_r(x[i + 1], x[i], s);
    x[K - 1] = funnel_r(0u, x[K - 1], s);
}
// x << words * 32 + bits and back, words < 16, bits < 32, both per lane
template <int K>
KZG_DEV void w_shl_var(wv<K>& x, uint32_t words, uint32_t bits) {
    w_up<K, 1>(x, words & 1u);
    w_up<K, 2>(x, words & 2u);
    if (K > 4) w_up<K, 4>(x, words & 4u);
    if (K > 8) w_up<K, 8>(x, words & 8u);
    w_shl_bits<K>(x, bits);
}
template <int K>
KZG_DEV void w_shr_var(wv<K>& x, uint32_t words, uint32_t bits) {
    w_down<K, 1>(x, words & 1u);
    w_down<K, 2>(x, words & 2u);
    if (K > 4) w_down<K, 4>(x, words & 4u);
    if (K > 8) w_down<K, 8>(x, words & 8u);
    w_shr_bits<K>(x, bits);
}
// x << b and x >> b for the limb width 1 <= b <= 64 (uniform over the workgroup)
template <int K>
KZG_DEV void w_shl_limb(wv<K>& x, uint32_t b) {
    if (b == 64) {
        w_up<K, 2>(x, true);
    } else {
        if (b >= 32) w_up<K, 1>(x, true);
        w_shl_bits<K>(x, b & 31u);
    }
}
template <int K>
KZG_DEV void w_shr_limb(wv<K>& x, uint32_t b) {
    if (b == 64) {
        w_down<K, 2>(x, true);
    } else {
        if (b >= 32) w_down<K, 1>(x, true);
        w_shr_bits<K>(x, b & 31u);
    }
}
template <int K>
KZG_DEV bool w_nonzero(const wv<K>& x) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < K; i++) o |= x[i];
    return o != 0;
}
// a > b
template <int K>
KZG_DEV bool w_gt(const wv<K>& a, const wv<K>& b) {
    uint32_t br = 0;   // the borrow of b - a
#pragma unroll
    for (int i = 0; i < K; i++) {
        const uint64_t d = (uint64_t)b[i] - a[i] - br;
        br = (uint32_t)(d >> 32) & 1u;
    }
    return br != 0;
}
// r <- a + b, returns the carry out; r <- a - b, returns the borrow out
template <int K>
KZG_DEV uint32_t w_add(wv<K>& r, const wv<K>& a, const wv<K>& b) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const uint64_t s = (uint64_t)a[i] + b[i] + c;
        r[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return c;
}
template <int K>
KZG_DEV uint32_t w_sub(wv<K>& r, const wv<K>& a, const wv<K>& b) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - br;
        r[i] = (uint32_t)d;
        br = (uint32_t)(d >> 32) & 1u;
    }
    return br;
}
// p <- a b + d, the schoolbook product by rows (a b + d < 2^(64 N): it cannot overflow)
template <int N>
KZG_DEV void w_mul_add(wv<2 * N>& p, const wv<N>& a, const wv<N>& b, const wv<N>& d) {
#pragma unroll
    for (int i = 0; i < N; i++) {
        p[i] = d[i];
        p[N + i] = 0;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t s = (uint64_t)a[i] * b[j] + p[i + j] + c;   // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            p[i + j] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
        p[i + N] = c;
    }
}

// ---- Knuth D: u = q v + r with r < v, for v != 0.  U = u << s (3 N words; its top word is below 2^31) against V = v << s with
// bit 32 N - 1 set.  The 2 N digit steps ROLL: each works on the window U[2N-1 .. 3N-1], whose top word its step clears, then
// U moves up one word and the digit enters q from below -- constant indices without unrolling 2 N steps of N products
template <int N>
KZG_DEV void w_divrem(wv<2 * N>& q, wv<N>& r, const wv<2 * N>& u, const wv<N>& v) {
    wv<N> V;
    wv<3 * N> U;
    uint32_t lzw = 0, top = 0;   // the zero words above v's top word, and that word
    bool seen = false;
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        const bool nz = v[i] != 0;
        lzw += (!seen && !nz) ? 1u : 0u;
        top = (!seen && nz) ? v[i] : top;
        seen |= nz;
    }
    const uint32_t lzb = (uint32_t)__clz((int)(top | 1u)) & 31u;   // (v != 0: top != 0; the | 1 keeps __clz defined anyway)
#pragma unroll
    for (int i = 0; i < N; i++) V[i] = v[i];
#pragma unroll
    for (int i = 0; i < 3 * N; i++) U[i] = i < 2 * N ? u[i < 2 * N ? i : 0] : 0u;
    w_shl_var<N>(V, lzw, lzb);
    w_shl_var<3 * N>(U, lzw, lzb);
    const uint32_t d1 = V[N - 1] | 0x80000000u, d0 = V[N - 2];   // (the top bit is set already where v != 0)
    const uint32_t dinv = (uint32_t)(~0ull / d1);                // floor((2^64 - 1) / d1) - 2^32
    w_zero<2 * N>(q);
#pragma unroll 1
    for (int step = 0; step < 2 * N; step++) {
        constexpr int J = 2 * N - 1;   // the window's lowest word
        const uint32_t u2 = U[J + N], u1 = U[J + N - 1], u0 = U[J + N - 2];
        // qhat = min(floor((u2 : u1) / d1), 2^32 - 1) and rhat = (u2 : u1) - qhat d1, which may pass 2^32 (u2 <= d1 always)
        const uint64_t e = (uint64_t)dinv * u2 + (((uint64_t)u2 << 32) | u1);
        uint32_t q1 = (uint32_t)(e >> 32) + 1u, rr = u1 - q1 * d1;
        if (rr > (uint32_t)e) {
            q1--;
            rr += d1;
        }
        if (rr >= d1) {
            q1++;
            rr -= d1;
        }
        const bool cap = u2 >= d1;
        uint32_t qhat = cap ? 0xffffffffu : q1;
        uint64_t rhat = cap ? (uint64_t)u1 + d1 : (uint64_t)rr;
#pragma unroll
        for (int rep = 0; rep < 2; rep++) {
            const bool fix = (rhat >> 32) == 0 && (uint64_t)qhat * d0 > ((rhat << 32) | u0);
            qhat -= fix ? 1u : 0u;
            rhat += fix ? d1 : 0u;
        }
        uint32_t c = 0, br = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint64_t p = (uint64_t)qhat * V[i] + c;
            c = (uint32_t)(p >> 32);
            const uint64_t d = (uint64_t)U[J + i] - (uint32_t)p - br;
            U[J + i] = (uint32_t)d;
            br = (uint32_t)(d >> 32) & 1u;
        }
        br = (uint32_t)(((uint64_t)u2 - c - br) >> 32) & 1u;
        const uint32_t back = br ? 0xffffffffu : 0u;   // qhat was one too large: add V back
        c = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint64_t s = (uint64_t)U[J + i] + (V[i] & back) + c;
            U[J + i] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
        // (the window's top word is 0 now: the remainder is below V)  U and q one word up, the digit in
#pragma unroll
        for (int i = 3 * N - 1; i >= 1; i--) U[i] = U[i - 1];
        U[0] = 0;
#pragma unroll
        for (int i = 2 * N - 1; i >= 1; i--) q[i] = q[i - 1];
        q[0] = qhat - br;
    }
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = U[2 * N + i];
    w_shr_var<N>(r, lzw, lzb);
}

// ---- cells in and out
// the vector of limb l of operand `which` of op, at row t
KZG_DEV const uint32_t* wide_cell(const WideTab& tab, const WideOp& op, int which, uint32_t l, uint64_t T, uint64_t t) {
    return tab.src + ((uint64_t)op.slot[which][l] * T + t) * 8;
}
// the limb l of a row, reduced to its low b bits; *over |= it was at or above 2^b
KZG_DEV uint64_t wide_limb(const uint32_t* p, uint64_t mask, bool* over) {
    bool high;
    const uint64_t raw = int_load(p, &high), x = raw & mask;
    *over |= high || x != raw;
    return x;
}
// x <- the wide operand `which`, packed from its top limb down
template <int N>
KZG_DEV void wide_load(wv<N>& x, const WideTab& tab, const WideOp& op, int which, uint64_t mask, uint64_t T, uint64_t t,
                       bool* over) {
    w_zero<N>(x);
#pragma unroll 1
    for (uint32_t l = op.limbs; l-- > 0;) {
        const uint64_t v = wide_limb(wide_cell(tab, op, which, l, T, t), mask, over);
        w_shl_limb<N>(x, op.bits);
        x[0] |= (uint32_t)v;
        x[1] |= (uint32_t)(v >> 32);
    }
}
// the eight limbs of operand `which`, pushed in from the top one down (y[l] = limb l; limbs at or above L stay 0)
KZG_DEV void limbs_load(uint64_t (&y)[WIDE_MAX_LIMBS], const WideTab& tab, const WideOp& op, int which, uint64_t mask, uint64_t T,
                        uint64_t t, bool* over) {
#pragma unroll
    for (int i = 0; i < WIDE_MAX_LIMBS; i++) y[i] = 0;
#pragma unroll 1
    for (uint32_t l = op.limbs; l-- > 0;) {
        const uint64_t v = wide_limb(wide_cell(tab, op, which, l, T, t), mask, over);
#pragma unroll
        for (int i = WIDE_MAX_LIMBS - 1; i >= 1; i--) y[i] = y[i - 1];
        y[0] = v;
    }
}
// the limbs of a packed value: y[l] = (x >> b l) mod 2^b for l < L, else 0
template <int N>
KZG_DEV void limbs_of(uint64_t (&y)[WIDE_MAX_LIMBS], wv<N>& x, uint32_t L, uint32_t b, uint64_t mask) {
#pragma unroll
    for (int i = 0; i < WIDE_MAX_LIMBS; i++) {
        y[i] = (uint32_t)i < L ? ((((uint64_t)x[1] << 32) | x[0]) & mask) : 0;
        if ((uint32_t)i < L) w_shr_limb<N>(x, b);
    }
}
// cnt limbs of x from the bottom up into the output vectors first, first + 1, ..; what is left of x stays in x
template <int K>
KZG_DEV void wide_store(uint32_t* out, uint32_t first, uint32_t cnt, wv<K>& x, uint32_t b, uint64_t mask, uint64_t T,
                        uint64_t t) {
#pragma unroll 1
    for (uint32_t l = 0; l < cnt; l++) {
        int_store(out + ((uint64_t)(first + l) * T + t) * 8, (((uint64_t)x[1] << 32) | x[0]) & mask);
        w_shr_limb<K>(x, b);
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_fr_wide(const WideTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st,
                                                  uint32_t n_ops) {
    const WideOp& op = tab.op[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = op.bits, L = op.limbs, kind = op.kind;
    const uint64_t mask = b == 64 ? ~0ull : (1ull << b) - 1;
    const bool has_b = op.flags & WIDE_F_ROW_B, has_c = op.flags & WIDE_F_ROW_C, neg_c = op.flags & KZG_WIDE_NEG_C;
    bool over = false, qover = false;
    if (t < n && kind <= KZG_WIDE_MUL) {   // KZG_WIDE_ADD, _SUB, _MUL
        wv<N> A, B;
        wide_load<N>(A, tab, op, WIDE_A, mask, T, t, &over);
        if (op.flags & WIDE_F_B_IS_A) {   // one run of rows as both operands: one load
#pragma unroll
            for (int i = 0; i < N; i++) B[i] = A[i];
        } else if (has_b) {
            wide_load<N>(B, tab, op, WIDE_B, mask, T, t, &over);
        } else {
#pragma unroll
            for (int i = 0; i < N; i++) B[i] = op.imm[i];
        }
        if (kind == KZG_WIDE_MUL) {
            wv<2 * N> P;
            wv<N> Z;
            w_zero<N>(Z);
            w_mul_add<N>(P, A, B, Z);
            wide_store<2 * N>(op.out, 0, op.count, P, b, mask, T, t);
        } else {
            // L limbs of the sum or difference mod 2^W, then one cell: the bit of the sum that is left above the L limbs (the
            // carry out of the N words where W = 32 N); the borrow out of the N words (both operands are below 2^W)
            wv<N> S;
            wv<N + 2> X;
            const uint32_t x = kind == KZG_WIDE_ADD ? w_add<N>(S, A, B) : w_sub<N>(S, A, B);
#pragma unroll
            for (int i = 0; i < N; i++) X[i] = S[i];
            X[N] = kind == KZG_WIDE_ADD ? x : 0u;
            X[N + 1] = 0;
            wide_store<N + 2>(op.out, 0, L, X, b, mask, T, t);
            if (op.count > L)
                int_store(op.out + ((uint64_t)L * T + t) * 8, kind == KZG_WIDE_ADD ? (uint64_t)(X[0] & 1u) : (uint64_t)x);
        }
    } else if (t < n) {   // KZG_WIDE_DIVMOD, _MULMOD, _CARRY: the kinds that divide
        wv<N> A, B, C, M, R;
        wv<2 * N> P, Q;
#pragma unroll
        for (int i = 0; i < N; i++) M[i] = op.m[i];
        w_zero<N>(C);
        if (has_c && (neg_c || kind != KZG_WIDE_CARRY)) wide_load<N>(C, tab, op, WIDE_C, mask, T, t, &over);
        const bool c_big = neg_c && w_gt<N>(C, M);   // out of range: counted, and reduced by the first pass
        over |= c_big;
        bool zero_div = false;
        if (kind != KZG_WIDE_CARRY) {
            wide_load<N>(A, tab, op, WIDE_A, mask, T, t, &over);
            if (op.flags & WIDE_F_B_IS_A) {
#pragma unroll
                for (int i = 0; i < N; i++) B[i] = A[i];
            } else if (has_b) {
                wide_load<N>(B, tab, op, WIDE_B, mask, T, t, &over);
            } else {
#pragma unroll
                for (int i = 0; i < N; i++) B[i] = op.imm[i];   // (absent: the host wrote 1)
            }
            zero_div = kind == KZG_WIDE_DIVMOD && !w_nonzero<N>(B);
        }
        // pass 0 (only where some lane of the wave has c > m): C <- C mod M.  pass 1: the division of the kind.  One body
#pragma unroll 1
        for (int pass = __any(c_big) ? 0 : 1; pass < 2; pass++) {
            wv<N> V;
            if (pass == 1 && neg_c) {   // d = m - (c mod m), in [1, m]: c = m is c mod m = 0
                const bool wrap = !w_gt<N>(M, C);
#pragma unroll
                for (int i = 0; i < N; i++) C[i] = wrap ? 0u : C[i];
                w_sub<N>(C, M, C);
            }
            if (pass == 1 && kind == KZG_WIDE_CARRY) break;
            if (pass == 0) {
#pragma unroll
                for (int i = 0; i < N; i++) {
                    P[i] = C[i];
                    P[N + i] = 0;
                    V[i] = M[i];
                }
            } else if (kind == KZG_WIDE_DIVMOD) {
#pragma unroll
                for (int i = 0; i < N; i++) {
                    P[i] = A[i];
                    P[N + i] = 0;
                    V[i] = B[i];
                }
                V[0] |= zero_div ? 1u : 0u;
            } else {
                w_mul_add<N>(P, A, B, C);
#pragma unroll
                for (int i = 0; i < N; i++) V[i] = M[i];
            }
            w_divrem<N>(Q, R, P, V);
            if (pass == 0) {
#pragma unroll
                for (int i = 0; i < N; i++) C[i] = c_big ? R[i] : C[i];
            }
        }
        if (kind == KZG_WIDE_DIVMOD) {   // floor(a / b) then a mod b; 2^W - 1 and a where b = 0
#pragma unroll
            for (int i = 0; i < N; i++) {
                Q[i] = zero_div ? 0xffffffffu : Q[i];
                R[i] = zero_div ? A[i] : R[i];
            }
            wide_store<2 * N>(op.out, 0, L, Q, b, mask, T, t);
            if (op.count > L) wide_store<N>(op.out, L, L, R, b, mask, T, t);
        } else if (kind == KZG_WIDE_MULMOD) {   // r then the low W bits of q; a q at or above 2^W is counted
            wide_store<N>(op.out, 0, L, R, b, mask, T, t);
            if (op.count > L) {
                wide_store<2 * N>(op.out, L, L, Q, b, mask, T, t);
            } else {
#pragma unroll 1
                for (uint32_t l = 0; l < L; l++) w_shr_limb<2 * N>(Q, b);
            }
            qover = w_nonzero<2 * N>(Q);
        } else {   // KZG_WIDE_CARRY: on the limbs themselves
            uint64_t a[WIDE_MAX_LIMBS], bb[WIDE_MAX_LIMBS], q[WIDE_MAX_LIMBS], r[WIDE_MAX_LIMBS], d[WIDE_MAX_LIMBS], m[WIDE_MAX_LIMBS];
            if (neg_c) {
                limbs_of<N>(d, C, L, b, mask);
            } else if (has_c) {
                limbs_load(d, tab, op, WIDE_C, mask, T, t, &over);
            } else {
#pragma unroll
                for (int i = 0; i < WIDE_MAX_LIMBS; i++) d[i] = 0;
            }
            limbs_of<N>(m, M, L, b, mask);
            limbs_load(a, tab, op, WIDE_A, mask, T, t, &over);
            if (has_b) {
                limbs_load(bb, tab, op, WIDE_B, mask, T, t, &over);
            } else {
#pragma unroll
                for (int i = 0; i < N; i++) B[i] = op.imm[i];
                limbs_of<N>(bb, B, L, b, mask);
            }
            limbs_load(q, tab, op, WIDE_Q, mask, T, t, &over);
            limbs_load(r, tab, op, WIDE_R, mask, T, t, &over);
            // s_k = sum_{i + j = k} (a_i b_j - q_i m_j) + [k < L] (d_k - r_k) + carry_{k - 1}; carry_k = floor(s_k / 2^b)
            // (the carries wait in cy and leave through ONE encoder body in a rolled loop below: cy[0] out, the rest one down)
            __int128 carry = 0;
            bool inexact = false;
            int64_t cy[2 * WIDE_MAX_LIMBS - 1];
#pragma unroll
            for (int k = 0; k < 2 * WIDE_MAX_LIMBS - 1; k++) {
                cy[k] = 0;
                if ((uint32_t)k < 2 * L - 1) {
                    __int128 s = carry;
#pragma unroll
                    for (int i = 0; i < WIDE_MAX_LIMBS; i++) {
                        constexpr int dummy = 0;
                        const int j = k - i;
                        if (j >= 0 && j < WIDE_MAX_LIMBS && (uint32_t)i < L && (uint32_t)j < L) {
                            const int jj = j >= 0 && j < WIDE_MAX_LIMBS ? j : dummy;
                            s += (__int128)((unsigned __int128)a[i] * bb[jj]);
                            s -= (__int128)((unsigned __int128)q[i] * m[jj]);
                        }
                    }
                    if (k < WIDE_MAX_LIMBS) {
                        const int kk = k < WIDE_MAX_LIMBS ? k : 0;
                        s += (__int128)d[kk] - (__int128)r[kk];
                    }
                    inexact |= ((uint64_t)s & mask) != 0;
                    carry = s >> b;   // (arithmetic, towards minus infinity; b <= 56, so |carry| < 2^63)
                    cy[k] = (int64_t)carry;
                }
            }
#pragma unroll 1
            for (uint32_t k = 0; k < op.count; k++) {
                const int64_t x = cy[0];
                int_store_signed(op.out + ((uint64_t)k * T + t) * 8, x < 0 ? 0ull - (uint64_t)x : (uint64_t)x, x < 0);
#pragma unroll
                for (int i = 0; i < 2 * WIDE_MAX_LIMBS - 2; i++) cy[i] = cy[i + 1];
            }
            qover = inexact || carry != 0;   // (s_{2L-1} = carry_{2L-2}: exact with carry_{2L-1} = 0 only where that is 0)
        }
    }
    derive_count(over, st + blockIdx.y);
    derive_count(qover, st + n_ops + blockIdx.y);
    expr_first(over, st + 2 * n_ops + blockIdx.y);
    expr_first(qover, st + 3 * n_ops + blockIdx.y);
}

void launch_wide(hipStream_t s, const WideTab& tab, uint32_t n_ops, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || n_ops == 0 || n_ops > WIDE_MAX_OPS || !tab.src) return;
    uint32_t words = 0;
    for (uint32_t o = 0; o < n_ops; o++) {
        const WideOp& op = tab.op[o];
        const uint32_t W = op.bits * op.limbs, maxc = op.kind == KZG_WIDE_CARRY ? 2 * op.limbs - 1 : 2 * op.limbs;
        if (!op.out || op.bits == 0 || op.bits > 64 || op.limbs == 0 || op.limbs > WIDE_MAX_LIMBS || W > 512 || op.count == 0 ||
            op.count > maxc || op.kind < KZG_WIDE_ADD || op.kind > KZG_WIDE_CARRY || (op.kind == KZG_WIDE_CARRY && op.bits > 56))
            return;
        words = (W + 31) / 32 > words ? (W + 31) / 32 : words;
    }
    const dim3 grid(nblk(n, 256), n_ops);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    if (words <= 4)
        k_fr_wide<4><<<grid, 256, 0, s>>>(tab, T, n, st, n_ops);
    else if (words <= 8)
        k_fr_wide<8><<<grid, 256, 0, s>>>(tab, T, n, st, n_ops);
    else
        k_fr_wide<16><<<grid, 256, 0, s>>>(tab, T, n, st, n_ops);
}
