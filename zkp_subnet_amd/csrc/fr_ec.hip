// fr_ec.hip -- Fr-side kernels, part 19: the non-native elliptic-curve columns of kzg_rows_commit_ec: a b^-1 mod p, the affine
// addition (lambda, x3, y3) of two points with the doubling, and the accumulator trace of a double-and-add chain, over an odd
// modulus p < 2^256 that is NOT the scalar field.  A WIDE VALUE is L <= 4 consecutive source columns of b <= 64 bits, packed into
// EC_WORDS = 8 words of 32 bits as in fr_wide.hip (from the top limb down, X <- (X << b) | limb); every limb cell is read as its
// canonical integer (int_load of fr_u64.hip.h) and reduced to its low b bits; an operand at or above p is reduced mod p.  A row
// with either is counted once.  Source columns lie as evaluation vectors of T elements of 8 words, Montgomery, canonical.
//   ONE launch per call, grid y = unit, 256 lanes per workgroup, ONE kernel k_fr_ec whose three unit forms branch on the unit's
//   mode, which is uniform over the workgroup.  The curve (p, a, -p^-1 mod 2^32, 2^512 mod p) rides in the kernel argument:
//   scalar loads, SGPRs.  A value is a VECTOR of 8 words (ev), never an array, so that every index is a compile-time constant
//   and nothing is addressed dynamically (fr_wide.hip has the reason).  No LDS, no barrier.
//   PRODUCTS mod p: Montgomery's, word by word (CIOS) at the fixed radix 2^256 whatever W is: 2 x 64 multiply-adds.  p odd is
//   what makes that radix invertible.  Values stay plain integers below p between the products: ec_mul(x, y) = x y mod p is two
//   products, the first by 2^512 mod p.
//   THE INVERSION: a binary extended GCD on (u, v) = (b, p) with v odd throughout.  One step: where u is odd, the larger of
//   (u, v) becomes u and u <- u - v (even); then u <- u / 2.  The cofactors A, C with u = A b, v = C b mod p follow: A <- A -
//   C mod p, A <- A / 2 mod p (A + p where A is odd).  Every step takes at least one bit off bits(u) + bits(v) <= 512, so the
//   loop ends within 512 steps, and it is capped there.  At u = 0, v = gcd(b, p): 1: C is the inverse; anything else (b = 0
//   included): the row is EXCEPTIONAL.  The step count differs from lane to lane; a wave runs as long as its slowest lane.
//   The step is written with selects, not branches, so that the lanes of a wave share one body.
//     a DIV unit     one lane per row t' < n: r = a b^-1.
//     an ADD unit    one lane per row: x1 != x2: lambda = (y2 - y1) / (x2 - x1); equal points: (3 x1^2 + a) / (2 y1); else the
//                    denominator stays 0 and the inversion reports the row.  ONE inversion per row.
//     a CHAIN unit   one lane per SEGMENT.  The lane of row t reads op[t]; where t = 0 or op[t] is a load it walks forward
//                    until the next load or n, the other lanes leave.  The lane that loads at t > 0 starts with the loaded
//                    point and writes rows t + 1 .. the next load's row; row t itself belongs to the lane before (it holds
//                    the accumulator before the load).  One segment over the whole column runs on ONE lane: a known limit
//                    (DESIGN.md has its measure).
//   Outputs leave as in fr_wide.hip: limb <- X mod 2^b, X <- X >> b, one int_store body.  In a check the same walk compares
//   the limb with the expected cell.  Statistics: a lane that met a flagged row adds to the unit's words with plain atomics
//   (such lanes are the exception, and the compiler folds the adds of a wave into one).
//   Registers (gfx950, the compiler's resource remarks): 134 VGPRs, no LDS, no scratch, 3 waves per SIMD; 82 scalar spills into
//   VGPR lanes (the unit table and the curve).  DESIGN.md has the table and the measured rates.
// Bound: compute.  An inversion is about 1.4 W steps of some 100 word operations, a product 128 multiply-adds; a row moves
// 32 B per limb cell in and out.
#include <cstring>

#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

typedef uint32_t ev __attribute__((ext_vector_type(EC_WORDS)));

// ---- words: every index a compile-time constant, every shift count below 32
KZG_DEV void e_zero(ev& x) {
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) x[i] = 0;
}
KZG_DEV bool e_is_zero(const ev& x) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) o |= x[i];
    return o == 0;
}
KZG_DEV bool e_eq(const ev& a, const ev& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) o |= a[i] ^ b[i];
    return o == 0;
}
// r <- a + b, returns the carry out; r <- a - b, returns the borrow out
KZG_DEV uint32_t e_add(ev& r, const ev& a, const ev& b) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) {
        const uint64_t s = (uint64_t)a[i] + b[i] + c;
        r[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return c;
}
KZG_DEV uint32_t e_sub(ev& r, const ev& a, const ev& b) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - br;
        r[i] = (uint32_t)d;
        br = (uint32_t)(d >> 32) & 1u;
    }
    return br;
}
// a < b
KZG_DEV bool e_lt(const ev& a, const ev& b) {
    ev d;
    return e_sub(d, a, b) != 0;
}
// x <- (c : x) >> 1, c the bit that enters from above
KZG_DEV void e_shr1(ev& x, uint32_t c) {
#pragma unroll
    for (int i = 0; i < EC_WORDS - 1; i++) x[i] = (x[i] >> 1) | (x[i + 1] << 31);
    x[EC_WORDS - 1] = (x[EC_WORDS - 1] >> 1) | (c << 31);
}
// x <- x << 1 | bit, returns the bit that leaves
KZG_DEV uint32_t e_shl1(ev& x, uint32_t bit) {
    const uint32_t top = x[EC_WORDS - 1] >> 31;
#pragma unroll
    for (int i = EC_WORDS - 1; i >= 1; i--) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
    x[0] = (x[0] << 1) | bit;
    return top;
}
// x << b and x >> b for the limb width 1 <= b <= 64 (uniform over the workgroup): whole words, then a funnel shift by b mod 32
// through a 64-bit intermediate, so that the counts 0, 32 and 64 meet no undefined shift
KZG_DEV void e_shl_limb(ev& x, uint32_t b) {
    const uint32_t words = b >> 5, s = b & 31u;
    if (words == 2) {
#pragma unroll
        for (int i = EC_WORDS - 1; i >= 0; i--) x[i] = i >= 2 ? x[i >= 2 ? i - 2 : 0] : 0u;
    } else if (words == 1) {
#pragma unroll
        for (int i = EC_WORDS - 1; i >= 0; i--) x[i] = i >= 1 ? x[i >= 1 ? i - 1 : 0] : 0u;
    }
#pragma unroll
    for (int i = EC_WORDS - 1; i >= 1; i--) x[i] = (uint32_t)(((((uint64_t)x[i] << 32) | x[i - 1]) << s) >> 32);
    x[0] = x[0] << s;
}
KZG_DEV void e_shr_limb(ev& x, uint32_t b) {
    const uint32_t words = b >> 5, s = b & 31u;
    if (words == 2) {
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) x[i] = i + 2 < EC_WORDS ? x[i + 2 < EC_WORDS ? i + 2 : 0] : 0u;
    } else if (words == 1) {
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) x[i] = i + 1 < EC_WORDS ? x[i + 1 < EC_WORDS ? i + 1 : 0] : 0u;
    }
#pragma unroll
    for (int i = 0; i < EC_WORDS - 1; i++) x[i] = (uint32_t)((((uint64_t)x[i + 1] << 32) | x[i]) >> s);
    x[EC_WORDS - 1] = x[EC_WORDS - 1] >> s;
}

// ---- the field of the call: plain integers below p
KZG_DEV void ec_p(ev& x, const EcTab& tab) {
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) x[i] = tab.p[i];
}
// r <- a + b mod p and a - b mod p, for a, b < p
KZG_DEV void ec_addm(ev& r, const ev& a, const ev& b, const EcTab& tab) {
    ev P, s, d;
    ec_p(P, tab);
    const uint32_t c = e_add(s, a, b);
    const uint32_t br = e_sub(d, s, P);
    const bool wrap = c || !br;   // a + b >= p
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) r[i] = wrap ? d[i] : s[i];
}
KZG_DEV void ec_subm(ev& r, const ev& a, const ev& b, const EcTab& tab) {
    ev P, s, d;
    ec_p(P, tab);
    const uint32_t br = e_sub(d, a, b);
    e_add(s, d, P);
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) r[i] = br ? s[i] : d[i];
}
// r <- a b / 2^256 mod p for a, b < p: Montgomery's product word by word.  The running sum (t8 : t) stays below 2 p
KZG_DEV void ec_mont(ev& r, const ev& a, const ev& b, const EcTab& tab) {
    ev t;
    e_zero(t);
    uint32_t t8 = 0;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < EC_WORDS; j++) {
            const uint64_t s = (uint64_t)a[i] * b[j] + t[j] + c;   // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            t[j] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
        uint64_t s = (uint64_t)t8 + c;
        t8 = (uint32_t)s;
        const uint32_t t9 = (uint32_t)(s >> 32);
        const uint32_t m = t[0] * tab.n0inv;
        s = (uint64_t)m * tab.p[0] + t[0];   // (its low word is 0)
        c = (uint32_t)(s >> 32);
#pragma unroll
        for (int j = 1; j < EC_WORDS; j++) {
            s = (uint64_t)m * tab.p[j] + t[j] + c;
            t[j - 1] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
        s = (uint64_t)t8 + c;
        t[EC_WORDS - 1] = (uint32_t)s;
        t8 = t9 + (uint32_t)(s >> 32);
    }
    ev P, d;
    ec_p(P, tab);
    const uint32_t br = e_sub(d, t, P);
    const bool wrap = t8 || !br;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) r[i] = wrap ? d[i] : t[i];
}
// r <- a b mod p: a 2^256 first (the product by 2^512 mod p), then the product with b
KZG_DEV void ec_mul(ev& r, const ev& a, const ev& b, const EcTab& tab) {
    ev R2, am;
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) R2[i] = tab.r2[i];
    ec_mont(am, a, R2, tab);
    ec_mont(r, am, b, tab);
}
// x <- x mod p for any x below 2^256, bit by bit from the top: r <- 2 r + bit, minus p where that reaches p.  256 steps: the
// path of the rows that are counted as out of range, and of an immediate at or above p
KZG_DEV void ec_reduce(ev& x, const EcTab& tab) {
    ev P, r, d;
    ec_p(P, tab);
    e_zero(r);
#pragma unroll 1
    for (int k = 0; k < 32 * EC_WORDS; k++) {
        const uint32_t bit = e_shl1(x, 0u);
        const uint32_t c = e_shl1(r, bit);
        const uint32_t br = e_sub(d, r, P);
        const bool wrap = c || !br;
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) r[i] = wrap ? d[i] : r[i];
    }
    x = r;
}
// r <- b^-1 mod p for b < p, returns whether it exists (gcd(b, p) = 1); r is 0 where it does not
KZG_DEV bool ec_inv(ev& r, const ev& b, const EcTab& tab) {
    ev P, u = b, v, A, C;
    ec_p(P, tab);
    v = P;
    e_zero(A);
    e_zero(C);
    A[0] = 1;
#pragma unroll 1
    for (int step = 0; step < 64 * EC_WORDS && !e_is_zero(u); step++) {
        const bool odd = u[0] & 1u;
        const bool sw = odd && e_lt(u, v);
        const uint32_t on = odd ? 0xffffffffu : 0u;
        ev vs, cs;
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) {
            const uint32_t tu = sw ? v[i] : u[i], tv = sw ? u[i] : v[i], ta = sw ? C[i] : A[i], tc = sw ? A[i] : C[i];
            u[i] = tu;
            v[i] = tv;
            A[i] = ta;
            C[i] = tc;
            vs[i] = tv & on;
            cs[i] = tc & on;
        }
        e_sub(u, u, vs);          // u odd: u >= v now, and u - v is even
        ec_subm(A, A, cs, tab);
        e_shr1(u, 0u);
        ev h;
        const uint32_t c = e_add(h, A, P);
        const bool a_odd = A[0] & 1u;
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) A[i] = a_odd ? h[i] : A[i];
        e_shr1(A, a_odd ? c : 0u);
    }
    ev one;
    e_zero(one);
    one[0] = 1;
    const bool ok = e_is_zero(u) && e_eq(v, one);
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) r[i] = ok ? C[i] : 0u;
    return ok;
}
// lambda, x3, y3 of (x1, y1) + (x2, y2), all below p; returns whether the row is exceptional (then the three are 0)
KZG_DEV bool ec_point_add(ev& lam, ev& x3, ev& y3, const ev& x1, const ev& y1, const ev& x2, const ev& y2, const EcTab& tab) {
    ev num, den, inv;
    ec_subm(den, x2, x1, tab);
    ec_subm(num, y2, y1, tab);
    if (e_is_zero(den) && e_is_zero(num)) {   // equal points: the tangent.  (Opposite points keep den = 0: no inverse)
        ev xx, a;
#pragma unroll
        for (int i = 0; i < EC_WORDS; i++) a[i] = tab.a[i];
        ec_addm(den, y1, y1, tab);
        ec_mul(xx, x1, x1, tab);
        ec_addm(num, xx, xx, tab);
        ec_addm(num, num, xx, tab);
        ec_addm(num, num, a, tab);
    }
    const bool ok = ec_inv(inv, den, tab);
    ec_mul(lam, inv, num, tab);   // (0 where there is no inverse)
    ev t;
    ec_mul(t, lam, lam, tab);
    ec_subm(t, t, x1, tab);
    ec_subm(x3, t, x2, tab);
    ec_subm(t, x1, x3, tab);
    ec_mul(t, lam, t, tab);
    ec_subm(y3, t, y1, tab);
#pragma unroll
    for (int i = 0; i < EC_WORDS; i++) {
        x3[i] = ok ? x3[i] : 0u;
        y3[i] = ok ? y3[i] : 0u;
    }
    return !ok;
}

// ---- cells in and out
// x <- the wide operand `which` of U at row t, packed from its top limb down and reduced mod p; *over |= a limb was at or above
// 2^b or the packed value at or above p
KZG_DEV void ec_load(ev& x, const EcTab& tab, const EcUnit& U, int which, uint64_t T, uint64_t t, bool* over) {
    const uint32_t b = tab.bits;
    const uint64_t mask = b == 64 ? ~0ull : (1ull << b) - 1;
    e_zero(x);
#pragma unroll 1
    for (uint32_t l = tab.limbs; l-- > 0;) {
        bool high;
        const uint64_t raw = int_load(tab.src + ((uint64_t)U.slot[which][l] * T + t) * 8, &high), v = raw & mask;
        *over |= high || v != raw;
        e_shl_limb(x, b);
        x[0] |= (uint32_t)v;
        x[1] |= (uint32_t)(v >> 32);
    }
    ev P;
    ec_p(P, tab);
    if (!e_lt(x, P)) {
        *over = true;
        ec_reduce(x, tab);
    }
}
// name k of U at row t: where it is an output, its L limbs into the unit's vectors; in a check, compared with the expected
// cells: *differs |= one of them is another integer
KZG_DEV void ec_emit(const EcTab& tab, const EcUnit& U, uint32_t k, ev x, uint64_t T, uint64_t t, bool* differs) {
    if (!(U.cols >> k & 1u)) return;
    const uint32_t b = tab.bits, L = tab.limbs, col = (uint32_t)__popc(U.cols & ((1u << k) - 1u)) * L;
    const uint64_t mask = b == 64 ? ~0ull : (1ull << b) - 1;
#pragma unroll 1
    for (uint32_t l = 0; l < L; l++) {
        const uint64_t w = (((uint64_t)x[1] << 32) | x[0]) & mask;
        if (U.out) {
            int_store(U.out + ((uint64_t)(col + l) * T + t) * 8, w);
        } else {
            bool high;
            const uint64_t e = int_load(tab.src + ((uint64_t)U.exp[k][l] * T + t) * 8, &high);
            *differs |= high || e != w;
        }
        e_shr_limb(x, b);
    }
}
// c flagged rows of a lane, the smallest of them `row`
KZG_DEV void ec_stat(uint32_t c, uint64_t row, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first) {
    if (!c) return;
    atomicAdd(cnt, (unsigned long long)c);
    atomicMin(first, (unsigned long long)row);
}

// one segment per lane: lane t < n of a CHAIN unit
KZG_DEV void ec_chain_unit(const EcTab& tab, const EcUnit& U, uint64_t T, uint64_t n, uint64_t t, unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const uint32_t* opv = tab.src + (uint64_t)U.opv * T * 8;
    bool high;
    const uint64_t c0 = int_load(opv + t * 8, &high);
    if (t != 0 && (high || c0 != 1)) return;   // no segment begins here
    atomicAdd(st + 3 * nu + u, 1ull);
    uint32_t n_over = 0, n_sing = 0, n_unk = 0;
    uint64_t f_over = ~0ull, f_sing = ~0ull, f_unk = ~0ull;
    ev ax, ay, zero;
    e_zero(zero);
    e_zero(ax);
    e_zero(ay);
    uint64_t s = 0;
    if (t != 0) {   // the load at t: row t itself is written by the lane of the segment before
        bool over = false;
        ec_load(ax, tab, U, 0, T, t, &over);
        ec_load(ay, tab, U, 1, T, t, &over);
        if (over) {
            n_over = 1;
            f_over = t;
        }
        s = t + 1;
    }
    bool unused = false;   // (a CHAIN unit is never a check)
#pragma unroll 1
    for (; s < n; s++) {
        const uint64_t raw = int_load(opv + s * 8, &high);
        const uint32_t code = high || raw > 3 ? 4u : (uint32_t)raw;
        ec_emit(tab, U, 0, ax, T, s, &unused);
        ec_emit(tab, U, 1, ay, T, s, &unused);
        if (code == 1 && s != 0) {   // the next segment: its lane takes over behind this row
            ec_emit(tab, U, 2, zero, T, s, &unused);
            break;
        }
        ev lam = zero;
        if (code == 4) {
            n_unk++;
            f_unk = f_unk < s ? f_unk : s;
        } else if (code != 0) {
            ev px = ax, py = ay;
            bool over = false;
            if (code != 3) {
                ec_load(px, tab, U, 0, T, s, &over);
                ec_load(py, tab, U, 1, T, s, &over);
            }
            if (over) {
                n_over++;
                f_over = f_over < s ? f_over : s;
            }
            if (code == 1) {
                ax = px;
                ay = py;
            } else {
                ev x3, y3;
                if (ec_point_add(lam, x3, y3, ax, ay, px, py, tab)) {
                    n_sing++;
                    f_sing = f_sing < s ? f_sing : s;
                }
                ax = x3;
                ay = y3;
            }
        }
        ec_emit(tab, U, 2, lam, T, s, &unused);
    }
    ec_stat(n_over, f_over, st + u, st + 4 * nu + u);
    ec_stat(n_sing, f_sing, st + nu + u, st + 5 * nu + u);
    ec_stat(n_unk, f_unk, st + 2 * nu + u, st + 6 * nu + u);
}

// T a power of two, n <= T; every slot, exp and opv that the unit's mode reads inside the source vectors (the launcher's and
// its caller's checks).  Lanes t >= n read nothing and store nothing
__global__ void __launch_bounds__(256) k_fr_ec(const EcTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    const EcUnit& U = tab.u[blockIdx.y];
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (U.mode == EC_CHAIN) {
        ec_chain_unit(tab, U, T, n, t, st);
        return;
    }
    bool over = false, differs = false, sing;
    if (U.mode == EC_DIV) {
        ev a, b, inv, r;
        ec_load(a, tab, U, 0, T, t, &over);
        if (U.flags & EC_F_IMM_B) {   // an immediate is reduced like a row, and not counted
            ev P;
            ec_p(P, tab);
#pragma unroll
            for (int i = 0; i < EC_WORDS; i++) b[i] = U.imm[i];
            if (!e_lt(b, P)) ec_reduce(b, tab);
        } else {
            ec_load(b, tab, U, 1, T, t, &over);
        }
        sing = !ec_inv(inv, b, tab);
        ec_mul(r, inv, a, tab);
        ec_emit(tab, U, 0, r, T, t, &differs);
    } else {
        ev x1, y1, x2, y2, lam, x3, y3;
        ec_load(x1, tab, U, 0, T, t, &over);
        ec_load(y1, tab, U, 1, T, t, &over);
        ec_load(x2, tab, U, 2, T, t, &over);
        ec_load(y2, tab, U, 3, T, t, &over);
        sing = ec_point_add(lam, x3, y3, x1, y1, x2, y2, tab);
        ec_emit(tab, U, 0, lam, T, t, &differs);
        ec_emit(tab, U, 1, x3, T, t, &differs);
        ec_emit(tab, U, 2, y3, T, t, &differs);
    }
    ec_stat(over, t, st + u, st + 4 * nu + u);
    ec_stat(sing, t, st + nu + u, st + 5 * nu + u);
    ec_stat(differs, t, st + 2 * nu + u, st + 6 * nu + u);
}

void launch_ec(hipStream_t s, const EcTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || tab.n_units == 0 || tab.n_units > EC_MAX_UNITS || !tab.src) return;
    if (tab.bits == 0 || tab.bits > 64 || tab.limbs == 0 || tab.limbs > EC_MAX_LIMBS || tab.bits * tab.limbs > 32 * EC_WORDS) return;
    bool p_big = false, a_small = false;   // p >= 3 and odd; a < p
    for (int i = EC_WORDS - 1; i >= 0; i--) {
        p_big |= i ? tab.p[i] != 0 : tab.p[0] >= 3;
        if (!a_small && tab.a[i] != tab.p[i]) {
            if (tab.a[i] > tab.p[i]) return;
            a_small = true;
        }
    }
    if (!p_big || !(tab.p[0] & 1u) || !a_small || tab.p[0] * tab.n0inv != 0xffffffffu) return;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const EcUnit& U = tab.u[u];
        if (U.mode != EC_DIV && U.mode != EC_ADD && U.mode != EC_CHAIN) return;
        const uint32_t names = U.mode == EC_DIV ? 1u : 7u, n_in = U.mode == EC_ADD ? 4u : 2u;
        if (!U.cols || (U.cols & ~names) || (U.mode == EC_CHAIN && (!U.out || U.opv >= POLY_MAX_ROWS))) return;
        for (uint32_t l = 0; l < tab.limbs; l++) {
            for (uint32_t w = 0; w < n_in; w++)
                if (U.slot[w][l] >= POLY_MAX_ROWS && !(w == 1 && (U.flags & EC_F_IMM_B))) return;
            for (uint32_t k = 0; k < 3; k++)
                if (!U.out && (U.cols >> k & 1u) && U.exp[k][l] >= POLY_MAX_ROWS) return;
        }
    }
    k_fr_ec<<<dim3(nblk(n, 256), tab.n_units), 256, 0, s>>>(tab, T, n, reinterpret_cast<unsigned long long*>(stats));
}
