// fr_edwards.hip -- Fr-side kernels, part 20: the native twisted-Edwards columns of kzg_rows_commit_edwards: the addition
// (x3, y3) of two pairs on A x^2 + y^2 = 1 + D x^2 y^2 over the scalar field ITSELF, and the accumulator trace of a
// double-and-add chain.  A coordinate is ONE cell: source columns lie as evaluation vectors of T elements of 8 words,
// Montgomery, canonical, and are used as the field elements they are (fr29.hip.h: nine 29-bit limbs).  With tau = D x1 x2 y1 y2
//     x3 = (x1 y2 + y1 x2) / (1 + tau)          y3 = (y1 y2 - A x1 x2) / (1 - tau)
// for every pair of pairs, equal ones included: there is no dedicated doubling, because one that substitutes the curve equation
// differs off the curve.  tau = +-1 is EXCEPTIONAL.
//   NO FIELD INVERSION runs in this file.  THREE steps per call (pipeline.hip, rows_edwards_dev):
//     k_edwards          ONE launch, grid y = unit, 256 lanes per workgroup, the unit forms branch on the unit's mode, which is
//                        uniform over the workgroup.  The unit table and the two curve constants ride in the kernel argument
//                        (scalar loads); A, D and the unit's up to four immediates are brought to Montgomery form once per
//                        workgroup into 6 x 9 words of LDS.
//       an ADD unit      one lane per row t < n: the numerators (x1 y2 + y1 x2)(1 - tau) and (y1 y2 - A x1 x2)(1 + tau) into
//                        the unit's output vectors, 1 - tau^2 into the unit's slice of the denominator vector Q.  9 products.
//                        On an exceptional row, and on the rows t >= n, Q takes Montgomery 1 (and an exceptional row's
//                        numerators 0): no zero reaches the inversion and no mask is needed.
//       an ADD check     stores nothing: expect_x (1 + tau) is compared with x1 y2 + y1 x2 and expect_y (1 - tau) with y1 y2 -
//                        A x1 x2; an exceptional row computes 0, so its expected cells must be 0.
//       a CHAIN unit     one lane per SEGMENT, found as k_fr_ec finds it: the lane of row t reads op[t]; where t = 0 or op[t]
//                        is a load it walks forward until the next load or n, the other lanes leave.  The lane that loads at
//                        t > 0 starts with the loaded point and writes rows t + 1 .. the next load's row; row t itself belongs
//                        to the lane before.  The lane holds (X : Y : Z) in registers; a step is the unified projective
//                        addition (Bernstein, Birkner, Joye, Lange, Peters 2008) with an affine second operand (Z2 = 1), 12
//                        products; the doubling is the same formula on (X : Y : Z) twice, 13.  Per row the lane stores X and Y
//                        into the named columns and Z into Q.  Z1 != 0 throughout, and Z3 = Z1^4 (1 - tau^2): Z3 = 0 (its
//                        canonical value) IS the exceptional step; the accumulator is then reset to (0 : 1 : 1) and counted.
//     the inversion      launch_fr_batch_inv (fr_lookup.hip), unchanged, over the (units with output) T elements of Q.
//     k_edwards_finish   out[c][t] <- out[c][t] W[unit(c)][t], canonical, for t < n.
//   Operand classes (fr29.hip.h).  Loaded cells and the LDS constants are canonical; every product leaves class N (< 2r, limbs
//   below 2^29).  Sums and differences stay lazy (the bounds are beside each line) and go into a product as its FIRST operand,
//   or through fr9_norm as its second.
//   Statistics: a lane that met a flagged row adds to the unit's words with plain atomics (such lanes are the exception).
//   Registers (gfx950, the compiler's resource remarks): k_edwards 147 VGPRs, 65 SGPRs, 216 B of LDS, no scratch,
//   no spills, 3 waves per SIMD; k_edwards_finish 50 VGPRs, no LDS, no scratch, 8 waves per SIMD.
// Bound: compute in k_edwards (a product is 153 multiply-adds; a row moves 32 B per cell), latency in a long segment
// (DESIGN.md has the measured rates).
#include <cstring>

#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

KZG_DEV bool fr9_is_zero(const fr9_t& a) {   // a canonical
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= a.l[i];
    return o == 0;
}
KZG_DEV bool fr9_differ(const fr9_t& a, const fr9_t& b) {   // both canonical
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= a.l[i] ^ b.l[i];
    return o != 0;
}
KZG_DEV void edw_lds(fr9_t& v, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 9; i++) v.l[i] = p[i];
}
// operand w (a compile-time constant) of U at row t: the cell, or the unit's immediate from LDS
KZG_DEV void edw_operand(fr9_t& v, const EdwTab& tab, const EdwUnit& U, int w, const uint32_t (*cst)[9], uint64_t T, uint64_t t) {
    if (U.slot[w] == EDW_IMM) edw_lds(v, cst[2 + w]);
    else fr9_load(v, tab.src + ((uint64_t)U.slot[w] * T + t) * 8);
}
// c flagged rows of a lane, the smallest of them `row`
KZG_DEV void edw_stat(uint32_t c, uint64_t row, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ first) {
    if (!c) return;
    atomicAdd(cnt, (unsigned long long)c);
    atomicMin(first, (unsigned long long)row);
}

// (X : Y : Z) <- (X : Y : Z) + (x2 : y2 : 1), or with dbl (X : Y : Z) + (X : Y : Z) (then x2 = X, y2 = Y are passed in).  X, Y,
// Z and x2, y2 normalised below 4r (class N, canonical, or a negated cell); the result is canonical
KZG_DEV void edw_padd(fr9_t& X, fr9_t& Y, fr9_t& Z, const fr9_t& x2, const fr9_t& y2, bool dbl, const fr9_t& Ac, const fr9_t& Dc) {
    fr9_t A = Z, B, C, D, E, F, G, m, s1, s2, f;
    if (dbl) fr9_mul(A, Z, Z);                // A = Z1 Z2
    fr9_mul(B, A, A);
    fr9_mul(C, X, x2);
    fr9_mul(D, Y, y2);
    fr9_mul(E, C, D);
    fr9_mul(E, E, Dc);                        // E = D-coefficient X1 X2 Y1 Y2
    fr9_add(s1, X, Y);                        // < 8r, limbs < 2^30
    fr9_add(s2, x2, y2);
    fr9_norm(s2, s2);                         // < 8r
    fr9_mul(m, s1, s2);                       // (X1 + Y1)(X2 + Y2)
    fr9_add(s1, C, D);
    fr9_norm(s1, s1);                         // < 4r
    fr9_sub8(m, m, s1);                       // X1 Y2 + Y1 X2, < 10r, limbs < 2^29 + 2^30
    fr9_mul(f, C, Ac);
    fr9_sub4(D, D, f);                        // Y1 Y2 - A X1 X2, < 6r
    fr9_sub4(F, B, E);                        // < 6r
    fr9_add(G, B, E);                         // < 4r
    fr9_mul(s1, F, A);                        // A F
    fr9_mul(s2, G, A);                        // A G
    fr9_mul(X, m, s1);
    fr9_mul(Y, D, s2);
    fr9_norm(G, G);
    fr9_mul(Z, F, G);
    fr9_canon(X, X);
    fr9_canon(Y, Y);
    fr9_canon(Z, Z);
}

// one segment per lane: lane t < n of a CHAIN unit
KZG_DEV void edw_chain_unit(const EdwTab& tab, const EdwUnit& U, const uint32_t (*cst)[9], uint64_t T, uint64_t n, uint64_t t,
                            unsigned long long* st) {
    const uint32_t nu = tab.n_units, u = blockIdx.y;
    const uint32_t* opv = tab.src + (uint64_t)U.opv * T * 8;
    bool high;
    const uint64_t c0 = int_load(opv + t * 8, &high);
    if (t != 0 && (high || c0 != 1)) return;   // no segment begins here
    atomicAdd(st + 2 * nu + u, 1ull);
    uint32_t n_sing = 0, n_unk = 0;
    uint64_t f_sing = ~0ull, f_unk = ~0ull;
    fr9_t X, Y, Z, one, Ac, Dc;
    fr9_one(one);
    edw_lds(Ac, cst[0]);
    edw_lds(Dc, cst[1]);
    fr9_zero(X);
    Y = one;
    Z = one;
    uint64_t s = 0;
    if (t != 0) {   // the load at t: row t itself is written by the lane of the segment before
        edw_operand(X, tab, U, 0, cst, T, t);
        edw_operand(Y, tab, U, 1, cst, T, t);
        s = t + 1;
    }
#pragma unroll 1
    for (; s < n; s++) {
        const uint64_t raw = int_load(opv + s * 8, &high);
        const uint32_t code = high || raw > 4 ? 5u : (uint32_t)raw;
        if (U.out[0]) fr9_store(U.out[0] + s * 8, X);
        if (U.out[1]) fr9_store(U.out[1] + s * 8, Y);
        fr9_store(U.q + s * 8, Z);
        if (code == 1 && s != 0) break;   // the next segment: its lane takes over behind this row
        if (code == 5) {
            n_unk++;
            f_unk = f_unk < s ? f_unk : s;
        } else if (code != 0) {
            fr9_t px = X, py = Y;
            if (code != 3) {
                edw_operand(px, tab, U, 0, cst, T, s);
                edw_operand(py, tab, U, 1, cst, T, s);
            }
            if (code == 1) {
                X = px;
                Y = py;
                Z = one;
            } else {
                if (code == 4) {   // -px: 4r - px, normalised, at most 4r
                    fr9_t z;
                    fr9_zero(z);
                    fr9_sub4(px, z, px);
                    fr9_norm(px, px);
                }
                edw_padd(X, Y, Z, px, py, code == 3, Ac, Dc);
                if (fr9_is_zero(Z)) {   // tau = +-1
                    n_sing++;
                    f_sing = f_sing < s ? f_sing : s;
                    fr9_zero(X);
                    Y = one;
                    Z = one;
                }
            }
        }
    }
    edw_stat(n_sing, f_sing, st + u, st + 3 * nu + u);
    edw_stat(n_unk, f_unk, st + nu + u, st + 4 * nu + u);
}

// T a power of two, n <= T; every slot, exp and opv that the unit's mode reads inside the source vectors (the launcher's and
// its caller's checks).  Lanes t >= n read nothing and store Montgomery 1 into Q, nothing else
__global__ void __launch_bounds__(256) k_edwards(const EdwTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ st) {
    __shared__ uint32_t cst[6][9];   // A, D, the unit's four immediates: Montgomery, canonical
    const EdwUnit& U = tab.u[blockIdx.y];
    const uint32_t nu = tab.n_units, u = blockIdx.y, lane = threadIdx.x;
    if (lane < 6) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t x = tab.a[i];
            x = lane == 1 ? tab.d[i] : x;
#pragma unroll
            for (int j = 0; j < 4; j++) x = lane == 2 + j ? U.imm[j][i] : x;
            w[i] = x;
        }
        fr9_t c;
        fr9_from_words(c, w);
        fr9_to_mont(c, c);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[lane][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + lane;
    if (t >= T) return;
    fr9_t one;
    fr9_one(one);
    if (t >= n) {
        if (U.q) fr9_store(U.q + t * 8, one);
        return;
    }
    if (U.mode == EDW_CHAIN) {
        edw_chain_unit(tab, U, cst, T, n, t, st);
        return;
    }
    fr9_t x1, y1, x2, y2, a, b, c, d, e, f, Ac, Dc;
    edw_operand(x1, tab, U, 0, cst, T, t);
    edw_operand(y1, tab, U, 1, cst, T, t);
    edw_operand(x2, tab, U, 2, cst, T, t);
    edw_operand(y2, tab, U, 3, cst, T, t);
    edw_lds(Ac, cst[0]);
    edw_lds(Dc, cst[1]);
    fr9_mul(a, x1, y2);
    fr9_mul(b, y1, x2);
    fr9_mul(c, x1, x2);
    fr9_mul(d, y1, y2);
    fr9_mul(e, c, d);
    fr9_mul(e, e, Dc);                        // tau
    fr9_mul(f, c, Ac);
    fr9_add(a, a, b);                         // x1 y2 + y1 x2, < 4r
    fr9_sub4(d, d, f);                        // y1 y2 - A x1 x2, < 6r
    fr9_sub4(b, one, e);                      // 1 - tau, < 5r
    fr9_add(c, one, e);                       // 1 + tau, < 3r
    fr9_norm(b, b);
    fr9_norm(c, c);
    fr9_mul(f, b, c);                         // 1 - tau^2
    fr9_canon(f, f);
    const bool sing = fr9_is_zero(f);
    bool differs = false;
    if (U.q) {
        fr9_mul(x1, a, b);
        fr9_mul(y1, d, c);
        fr9_canon(x1, x1);
        fr9_canon(y1, y1);
        if (sing) {
            fr9_zero(x1);
            fr9_zero(y1);
            f = one;
        }
        if (U.out[0]) fr9_store(U.out[0] + t * 8, x1);
        if (U.out[1]) fr9_store(U.out[1] + t * 8, y1);
        fr9_store(U.q + t * 8, f);
    } else {
        if (U.cols & 1u) {
            fr9_load(x2, tab.src + ((uint64_t)U.exp[0] * T + t) * 8);
            fr9_mul(y2, x2, c);               // expect_x (1 + tau)
            fr9_canon(y2, y2);
            fr9_reduce(a, a);
            differs |= sing ? !fr9_is_zero(x2) : fr9_differ(y2, a);
        }
        if (U.cols & 2u) {
            fr9_load(x2, tab.src + ((uint64_t)U.exp[1] * T + t) * 8);
            fr9_mul(y2, x2, b);               // expect_y (1 - tau)
            fr9_canon(y2, y2);
            fr9_reduce(d, d);
            differs |= sing ? !fr9_is_zero(x2) : fr9_differ(y2, d);
        }
    }
    edw_stat(sing, t, st + u, st + 3 * nu + u);
    edw_stat(differs, t, st + nu + u, st + 4 * nu + u);
}

// out[c][t] <- out[c][t] W[wq[c]][t] for t < n: the numerator (or the projective coordinate) times the inverted denominator
__global__ void __launch_bounds__(256) k_edwards_finish(const EdwFin fin, uint64_t T, uint64_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t* o = fin.out + ((uint64_t)blockIdx.y * T + t) * 8;
    fr9_t v, w;
    fr9_load(v, o);
    fr9_load(w, fin.W + ((uint64_t)fin.wq[blockIdx.y] * T + t) * 8);
    fr9_mul(v, v, w);
    fr9_canon(v, v);
    fr9_store(o, v);
}

void launch_edwards(hipStream_t s, const EdwTab& tab, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || tab.n_units == 0 || tab.n_units > EDW_MAX_UNITS || !tab.src) return;
    for (uint32_t u = 0; u < tab.n_units; u++) {
        const EdwUnit& U = tab.u[u];
        if (U.mode != EDW_ADD && U.mode != EDW_CHAIN) return;
        const uint32_t n_in = U.mode == EDW_ADD ? 4u : 2u;
        if (!U.cols || (U.cols & ~3u)) return;
        if (U.mode == EDW_CHAIN && (!U.q || U.opv >= POLY_MAX_ROWS)) return;
        if (U.q ? (!U.out[0] && !U.out[1]) : (U.out[0] || U.out[1])) return;
        for (uint32_t w = 0; w < n_in; w++)
            if (U.slot[w] >= POLY_MAX_ROWS && U.slot[w] != EDW_IMM) return;
        for (uint32_t k = 0; k < 2; k++)
            if (!U.q && (U.cols >> k & 1u) && U.exp[k] >= POLY_MAX_ROWS) return;
    }
    k_edwards<<<dim3(nblk(T, 256), tab.n_units), 256, 0, s>>>(tab, T, n, reinterpret_cast<unsigned long long*>(stats));
}

void launch_edwards_finish(hipStream_t s, const EdwFin& fin, uint32_t n_out, uint64_t T, uint64_t n) {
    if (!n || n > T || !n_out || n_out > POLY_MAX_ROWS || !fin.out || !fin.W) return;
    k_edwards_finish<<<dim3(nblk(n, 256), n_out), 256, 0, s>>>(fin, T, n);
}
