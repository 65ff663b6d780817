// fr_quot.hip -- Fr-side kernels, part 4: the PLONK quotient of kzg_rows_commit_quotient.  With T the row length, E = 2^ext_log
// and N = E T, the rows are evaluated on the coset g H_N (g = 7, H_N the N-th roots of unity, x_i = g w_N^i in natural
// order), the constraint arithmetic runs point by point there, and the result comes back to coefficients:
//   k_quot_consts   once per (T, E) and context: 1 / (x^T - 1) for the E values x^T takes on the coset, 1 / T, g, and the
//                   two-level power tables g^(+-i) = A[i mod 2^h] B[i >> h]  (h = ceil(log N / 2): two tables of ~sqrt N)
//   k_quot_extend   ext[i] = g^i f[i] (i < T), 0 above: the input of one forward transform of length N per row; with no row,
//                   the coefficients of L_0 (all 1 / T)
//   k_quot_points   one lane per coset point: (Gate + alpha P1 + alpha^2 P2) / Z_H; its second instantiation (kzg_rows_commit_
//                   quotient_ext) reads a gate factor at a rotation and adds alpha^3 LK1 + alpha^4 LK2, the logUp relation
//                   (kzg_rows_quotient_part with a link: P2 = (z - f_prev(w^rot X)) L_0, two instantiations more)
//   k_quot_accumulate   acc[i] (+)= scale v[i]: one part's num / Z_H into the accumulator of kzg_rows_quotient_part
//   k_quot_pieces   after the inverse transform: t[i] = g^-i v[i] for i < P T into the new set's buffer, the tail [P T, N)
//                   ORed into a flag word
// Z_H(x_i) = g^T w_E^(i mod E) - 1: E inversions per (T, E), none per point.  z(w x_i) = z at index (i + E) mod N, and in
// general f(w^rot x_i) = f's extended vector at index (i + rot E) mod N (w = w_N^E): a rotation costs no transform and no vector.
#include <cstring>

#include "fr_inv.hip.h"
#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// constants record (8-word Montgomery elements): [0, 8) 1 / Z_H by i mod E, [8] 1 / T, [9] g, [16, ..) the power tables
#define QC_INVT 8
#define QC_G 9
#define QC_TABLES 16
__host__ __device__ static inline int quot_h(int log_n) { return (log_n + 1) / 2; }
uint64_t quot_consts_elems(int log_t, int ext_log) {
    const int log_n = log_t + ext_log, h = quot_h(log_n);
    return QC_TABLES + 2 * (((uint64_t)1 << h) + ((uint64_t)1 << (log_n - h)));
}

KZG_DEV void fr9_pow(fr9_t& out, const fr9_t& base, uint64_t e) {   // canonical base -> canonical base^e
    fr9_t cur, pw = base;
    fr9_one(cur);
    for (; e; e >>= 1) {
        if (e & 1) fr9_mul(cur, cur, pw);
        fr9_mul(pw, pw, pw);
    }
    fr9_canon(out, cur);
}
KZG_DEV void fr9_coset_gen(fr9_t& g, int inverse) {   // g = 7 or 7^-1 mod r, Montgomery form
    constexpr uint32_t GI[8] = {0x24924925u, 0xdb6db6dbu, 0x49241a48u, 0xaa362edcu,
                                0x7077624au, 0x57c7624bu, 0xe7519182u, 0x211f5460u};
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = inverse ? GI[i] : (i == 0 ? 7u : 0u);
    fr9_from_words(g, t);
    fr9_to_mont(g, g);
}
KZG_DEV void tw_get(fr9_t& w, const uint32_t* __restrict__ tw, uint64_t k) {   // the NTT's twiddle slots: nine limbs in 48 bytes
    const uint4* q = reinterpret_cast<const uint4*>(tw + 12 * k);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
    w.l[0] = q0.x; w.l[1] = q0.y; w.l[2] = q0.z; w.l[3] = q0.w;
    w.l[4] = q1.x; w.l[5] = q1.y; w.l[6] = q1.z; w.l[7] = q1.w;
    w.l[8] = q2.x;
}

// ------------------------------------------------------------------------------------------------ constants
// tw: the forward twiddle table of length N (w_N^k, k < N / 2).  One lane per element of the record.
__global__ void __launch_bounds__(64) k_quot_consts(uint32_t* __restrict__ qc, int log_t, int ext_log,
                                                     const uint32_t* __restrict__ tw) {
    const int log_n = log_t + ext_log, h = quot_h(log_n);
    const uint64_t SA = (uint64_t)1 << h, SB = (uint64_t)1 << (log_n - h), half = (uint64_t)1 << (log_n - 1);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t E = 1u << ext_log;
    fr9_t v;
    if (t < E) {   // 1 / (g^T w_E^t - 1), w_E^t = w_N^(t T)
        fr9_t g, w, one;
        fr9_coset_gen(g, 0);
        fr9_pow(g, g, (uint64_t)1 << log_t);
        const uint64_t idx = t << log_t;
        tw_get(w, tw, idx & (half - 1));
        fr9_mul(v, g, w);
        if (idx >= half) {   // w_N^(idx) = -w_N^(idx - N/2)
            fr9_t z;
            fr9_zero(z);
            fr9_sub4(v, z, v);
        }
        fr9_one(one);
        fr9_sub4(v, v, one);
        fr9_reduce(v, v);
        (void)fr9_inv(v, v);   // never zero: g^T is not an E-th root of unity
    } else if (t < QC_INVT) {
        fr9_zero(v);
    } else if (t == QC_INVT) {
        constexpr uint32_t HALF[8] = {0x80000001u, 0x7fffffffu, 0x7fff2dffu, 0xa9ded201u,
                                      0x04d0ec02u, 0x199cec04u, 0x94cebea4u, 0x39f6d3a9u};   // (r + 1) / 2
        uint32_t hw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) hw[i] = HALF[i];
        fr9_from_words(v, hw);
        fr9_to_mont(v, v);
        fr9_pow(v, v, (uint64_t)log_t);
    } else if (t == QC_G) {
        fr9_coset_gen(v, 0);
    } else if (t < QC_TABLES) {
        fr9_zero(v);
    } else {
        const uint64_t u = t - QC_TABLES;
        if (u >= 2 * (SA + SB)) return;
        const int inverse = u >= SA + SB;
        const uint64_t e = inverse ? u - (SA + SB) : u;
        fr9_coset_gen(v, inverse);
        fr9_pow(v, v, e < SA ? e : (e - SA) << h);
    }
    fr9_store(qc + 8 * t, v);
}
void launch_quot_consts(hipStream_t s, uint32_t* qc, int log_t, int ext_log, const uint32_t* tw_n) {
    k_quot_consts<<<nblk(quot_consts_elems(log_t, ext_log), 64), 64, 0, s>>>(qc, log_t, ext_log, tw_n);
}

// g^(+-i) from the two tables: one product
KZG_DEV void quot_gpow(fr9_t& p, const uint32_t* __restrict__ qc, int log_n, int inverse, uint64_t i) {
    const int h = quot_h(log_n);
    const uint64_t SA = (uint64_t)1 << h, SB = (uint64_t)1 << (log_n - h);
    const uint32_t* tab = qc + 8 * (QC_TABLES + (inverse ? SA + SB : 0));
    fr9_t a, b;
    fr9_load(a, tab + 8 * (i & (SA - 1)));
    fr9_load(b, tab + 8 * (SA + (i >> h)));
    fr9_mul(p, a, b);
}

// ------------------------------------------------------------------------------------------------ coset extension
__global__ void __launch_bounds__(256) k_quot_extend(const uint32_t* __restrict__ f, uint32_t* __restrict__ ext, int log_t,
                                                      int log_n, const uint32_t* __restrict__ qc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    if (i >> log_t) {
        uint4* q = reinterpret_cast<uint4*>(ext + 8 * i);
        q[0] = make_uint4(0u, 0u, 0u, 0u);
        q[1] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    fr9_t p, c;
    quot_gpow(p, qc, log_n, 0, i);
    fr9_load(c, f ? f + 8 * i : qc + 8 * QC_INVT);
    fr9_mul(p, p, c);
    fr9_canon(p, p);
    fr9_store(ext + 8 * i, p);
}
void launch_quot_extend(hipStream_t s, const uint32_t* f_or_null, uint32_t* ext, int log_t, int ext_log, const uint32_t* qc) {
    const int log_n = log_t + ext_log;
    k_quot_extend<<<nblk((uint64_t)1 << log_n, 256), 256, 0, s>>>(f_or_null, ext, log_t, log_n, qc);
}

// ------------------------------------------------------------------------------------------------ the constraint arithmetic
// Everything that describes the constraints rides in ONE kernel argument (1.1 KB); the first lanes of every workgroup convert
// the scalars to Montgomery form once into LDS (one or two products each, in parallel).  The term loop is uniform over the
// workgroup (trip counts and row indices come from the argument), so a row pointer is a scalar load and a factor costs one
// 32-byte vector load and one product.  Sums are renormalised after every term: at most 16 terms + alpha P1 + alpha^2 P2,
// each below 2r, stay below 36r -- a legal first operand of the closing product by 1 / Z_H.
struct QuotArg {
    FrArg c[QUOT_MAX_TERMS], shift[QUOT_MAX_WIRES], beta, gamma, alpha;
    uint8_t len[QUOT_MAX_TERMS], row[QUOT_MAX_TERMS][QUOT_MAX_FACTORS], wire[QUOT_MAX_WIRES], sigma[QUOT_MAX_WIRES];
    uint32_t n_terms, k, z_row, ext_log;
};
static_assert(sizeof(QuotArg) + sizeof(RowTab) + 64 <= 4096, "k_quot_points' arguments must fit in 4 KB");
// What kzg_rows_commit_quotient_ext adds (1.8 KB in all): a rotation per gate factor, prepared on the host as (rot mod T) E so
// that the device does one add and one mask, and the lookup part.  The plain call keeps QuotArg and its own instantiation.
struct QuotArgX {
    QuotArg q;
    FrArg theta, lbeta;
    uint32_t rot[QUOT_MAX_TERMS][QUOT_MAX_FACTORS];
    uint8_t in_row[POLY_MAX_ROWS], tab_row[POLY_MAX_ROWS];
    uint32_t n_lookups, width, mult_row, sum_row;
};
static_assert(sizeof(QuotArgX) + sizeof(RowTab) + 64 <= 4096, "k_quot_points' arguments must fit in 4 KB");
// What kzg_rows_commit_quotient_zk adds: the row of the caller's fixed column A (1 on the usable rows, 0 elsewhere), a factor
// of P1 and of LK1.  The third instantiation's own argument: the two others keep theirs.
struct QuotArgA {
    QuotArgX x;
    uint32_t active_row;
};
static_assert(sizeof(QuotArgA) + sizeof(RowTab) + 64 <= 4096, "k_quot_points' arguments must fit in 4 KB");
// What a link of kzg_rows_quotient_part adds: the row of f_prev and its rotation, prepared on the host as (rot mod T) E like a
// gate factor's.  The linked instantiations' own argument: the three others keep theirs.
struct QuotArgL {
    QuotArgA a;
    uint32_t link_row, link_rot;
};
static_assert(sizeof(QuotArgL) + sizeof(RowTab) + 64 <= 4096, "k_quot_points' arguments must fit in 4 KB");
// What the _sel calls add (kzg_rows_commit_quotient_sel, kzg_rows_quotient_part_sel): per lookup the row of its selector q_l,
// the numerator of its fraction in LK1, or QUOT_NO_SEL (the constant 1).  The widest argument plus 16 bytes, for the SEL
// kernel alone: the five others keep theirs.
#define QUOT_NO_SEL 0xffu
struct QuotArgS {
    QuotArgL l;
    uint8_t sel_row[POLY_MAX_ROWS];
};
static_assert(sizeof(QuotArgS) + sizeof(RowTab) + 64 <= 4096, "k_quot_points_sel's arguments must fit in 4 KB");
template <bool EXT, bool ACT, bool LINK = false> struct QuotArgOf { typedef QuotArg type; };
template <> struct QuotArgOf<true, false, false> { typedef QuotArgX type; };
template <> struct QuotArgOf<true, true, false> { typedef QuotArgA type; };
template <bool ACT> struct QuotArgOf<true, ACT, true> { typedef QuotArgL type; };
KZG_DEV const QuotArg& quot_base(const QuotArg& a) { return a; }
KZG_DEV const QuotArg& quot_base(const QuotArgX& a) { return a.q; }
KZG_DEV const QuotArg& quot_base(const QuotArgA& a) { return a.x.q; }
KZG_DEV const QuotArg& quot_base(const QuotArgL& a) { return a.a.x.q; }
KZG_DEV const QuotArg& quot_base(const QuotArgS& a) { return a.l.a.x.q; }
KZG_DEV const QuotArg& quot_ext(const QuotArg& a) { return a; }
KZG_DEV const QuotArgX& quot_ext(const QuotArgX& a) { return a; }
KZG_DEV const QuotArgX& quot_ext(const QuotArgA& a) { return a.x; }
KZG_DEV const QuotArgX& quot_ext(const QuotArgL& a) { return a.a.x; }
KZG_DEV const QuotArgX& quot_ext(const QuotArgS& a) { return a.l.a.x; }
KZG_DEV uint32_t quot_active_row(const QuotArgS& a) { return a.l.a.active_row; }
KZG_DEV uint32_t quot_active_row(const QuotArgA& a) { return a.active_row; }
KZG_DEV uint32_t quot_active_row(const QuotArgL& a) { return a.a.active_row; }
enum { QS_SHIFT = QUOT_MAX_TERMS, QS_BETA = QS_SHIFT + QUOT_MAX_WIRES, QS_GAMMA, QS_ALPHA, QS_ALPHA2, QS_COUNT,
       QX_THETA = QS_COUNT, QX_LBETA, QX_ALPHA3, QX_ALPHA4, QX_COUNT };   // (the QX_ slots: the second instantiation only)
KZG_DEV void quot_arg(fr9_t& v, const FrArg& a, uint32_t* __restrict__ bad, bool check) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(a.w[7 - i]);
    if (check && fr_words_ge_r(w)) atomicOr(bad, 1u);
    fr9_from_words(v, w);
    fr9_to_mont(v, v);
}
KZG_DEV void lds_get(fr9_t& v, const uint32_t (*cst)[9], uint32_t j) {
#pragma unroll
    for (int i = 0; i < 9; i++) v.l[i] = cst[j][i];
}
// beta + sum_c theta^c f_c(x_i) over the w rows named by `rows`, Horner from the last column down: w - 1 products.  Every
// step is (a product, < 2r) + (a canonical row value, < r) < 3r with limbs < 2^30, a legal first operand of the next; the sum
// with beta stays below 4r (limbs < 2^31) and is normalised: a legal SECOND operand for a first one below 17r.
KZG_DEV void quot_lk_den(fr9_t& d, const RowTab& rt, const uint8_t* rows, uint32_t w, uint64_t i, const fr9_t& theta,
                         const fr9_t& beta) {
    fr9_t c;
    fr9_load(d, rt.r[rows[w - 1]] + 8 * i);
    for (uint32_t k = w - 1; k-- > 0;) {
        fr9_mul(d, d, theta);
        fr9_load(c, rt.r[rows[k]] + 8 * i);
        fr9_add(d, d, c);
    }
    fr9_add(d, d, beta);
    fr9_norm(d, d);
}
// EXT = false is kzg_rows_commit_quotient's kernel, instruction for instruction what it was before the second instantiation
// existed; EXT = true adds the rotations and the lookup part.  The lazy-sum bound with the lookup: at most 16 terms + alpha P1 +
// alpha^2 P2 + alpha^3 LK1 + alpha^4 LK2, each a product's output below 2r and the sum renormalised after each, stay below 40r --
// still under the 64r the closing product's first operand allows (its second one, 1 / Z_H, is canonical).
// ACT = true (with EXT; kzg_rows_commit_quotient_zk) is the third instantiation: num = Gate + alpha A P1 + alpha^2 P2 + alpha^3 A
// LK1 + alpha^4 LK2 with A the extended vector of the caller's active column.  A(x_i) is a canonical row value (the forward
// transform ends in fr9_reduce): a legal SECOND operand.  P1 is below 6r and LK1 below 10r, legal FIRST operands as they are for
// the products by alpha and alpha^3 that follow; A P1 and A LK1 come out below 2r, so those products and the lazy sum keep the
// bounds above.  One more 32-byte load and two more products per point; the two other instantiations keep their instructions.
// LINK = true (with EXT; kzg_rows_quotient_part with a link) replaces the 1 of P2 by f_prev(w^rot x_i), a canonical row value
// read like a rotated gate factor: z - f_prev through fr9_sub4 is below 5r exactly as z - 1 was, a legal first operand of the
// product by L_0, so P2 and the lazy sum keep the bounds above.  One more 32-byte load per point, in two instantiations of
// their own (with and without the active column, whose slot of the argument is simply not read); the three others keep their
// instructions.
template <bool EXT, bool ACT = false, bool LINK = false>
__global__ void __launch_bounds__(256) k_quot_points(const RowTab rt, const uint32_t* __restrict__ l0, uint32_t* __restrict__ out,
                                                      int log_n, const typename QuotArgOf<EXT, ACT, LINK>::type qarg,
                                                      const uint32_t* __restrict__ tw, const uint32_t* __restrict__ qc,
                                                      uint32_t* __restrict__ bad) {
    static_assert(EXT || !ACT, "the active column comes with the extended argument");
    static_assert(EXT || !LINK, "the link comes with the extended argument");
    const auto& qx = quot_ext(qarg);   // (the plain argument itself when !EXT: nothing of it is read through qx then)
    const QuotArg& qa = quot_base(qarg);
    __shared__ uint32_t cst[EXT ? QX_COUNT : QS_COUNT][9];
    const uint32_t v = threadIdx.x;
    const bool chk = blockIdx.x == 0;
    if (v < QS_COUNT) {
        fr9_t c;
        bool live = true;
        if (v < QS_SHIFT) {
            live = v < qa.n_terms;
            if (live) quot_arg(c, qa.c[v], bad, chk);
        } else if (v < QS_BETA) {   // beta s_j
            live = v - QS_SHIFT < qa.k;
            if (live) {
                fr9_t b;
                quot_arg(c, qa.shift[v - QS_SHIFT], bad, chk);
                quot_arg(b, qa.beta, bad, false);
                fr9_mul(c, c, b);
                fr9_canon(c, c);
            }
        } else if (v == QS_BETA) {
            quot_arg(c, qa.beta, bad, chk);
        } else if (v == QS_GAMMA) {
            quot_arg(c, qa.gamma, bad, chk);
        } else {
            quot_arg(c, qa.alpha, bad, chk);
            if (v == QS_ALPHA2) {
                fr9_mul(c, c, c);
                fr9_canon(c, c);
            }
        }
        if (!live) fr9_zero(c);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
    }
    if constexpr (EXT) {
        if (v >= QS_COUNT && v < QX_COUNT) {   // theta, the lookup's beta, alpha^3, alpha^4: one lane each
            fr9_t c;
            if (v == QX_THETA) {
                quot_arg(c, qx.theta, bad, chk);
            } else if (v == QX_LBETA) {
                quot_arg(c, qx.lbeta, bad, chk);
            } else {
                fr9_t a2;
                quot_arg(c, qa.alpha, bad, false);
                fr9_mul(a2, c, c);
                fr9_canon(a2, a2);
                fr9_mul(c, v == QX_ALPHA3 ? c : a2, a2);
                fr9_canon(c, c);
            }
#pragma unroll
            for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
        }
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + v;
    if (i >> log_n) return;
    const uint64_t n = (uint64_t)1 << log_n, half = n >> 1;
    fr9_t acc, p, c;
    [[maybe_unused]] fr9_t act;
    if constexpr (ACT) {
        if (qa.k || qx.n_lookups) fr9_load(act, rt.r[quot_active_row(qarg)] + 8 * i);
    }
    fr9_zero(acc);
    for (uint32_t u = 0; u < qa.n_terms; u++) {
        lds_get(p, cst, u);
        const uint32_t len = qa.len[u];
        for (uint32_t f = 0; f < len; f++) {
            if constexpr (EXT) fr9_load(c, rt.r[qa.row[u][f]] + 8 * ((i + qx.rot[u][f]) & (n - 1)));
            else fr9_load(c, rt.r[qa.row[u][f]] + 8 * i);
            fr9_mul(p, p, c);
        }
        fr9_add(acc, acc, p);
        fr9_norm(acc, acc);
    }
    if (qa.k) {
        fr9_t x, g, gamma, beta, A, B, z, a, sg, t, fa;
        // x_i = g w_N^i, kept lazy (a first operand only)
        fr9_load(g, qc + 8 * QC_G);
        tw_get(c, tw, i & (half - 1));
        fr9_mul(x, g, c);
        if (i >= half) {
            fr9_zero(t);
            fr9_sub4(x, t, x);
        }
        lds_get(gamma, cst, QS_GAMMA);
        lds_get(beta, cst, QS_BETA);
        const uint32_t* zr = rt.r[qa.z_row];
        fr9_load(z, zr + 8 * i);
        fr9_load(B, zr + 8 * ((i + ((uint64_t)1 << qa.ext_log)) & (n - 1)));
        A = z;
        for (uint32_t j = 0; j < qa.k; j++) {
            fr9_load(a, rt.r[qa.wire[j]] + 8 * i);
            fr9_load(sg, rt.r[qa.sigma[j]] + 8 * i);
            lds_get(c, cst, QS_SHIFT + j);
            fr9_mul(t, x, c);                 // beta s_j x_i
            fr9_add(fa, a, gamma);
            fr9_add(t, t, fa);                // < 4r
            fr9_norm(t, t);
            fr9_mul(A, t, A);
            fr9_mul(t, sg, beta);
            fr9_add(t, t, fa);
            fr9_norm(t, t);
            fr9_mul(B, t, B);
        }
        fr9_sub4(A, A, B);                    // P1, < 6r
        if constexpr (ACT) fr9_mul(A, A, act);   // A P1, < 2r
        lds_get(c, cst, QS_ALPHA);
        fr9_mul(t, A, c);
        fr9_add(acc, acc, t);
        fr9_norm(acc, acc);
        // P2 / Z_H = (z - 1) L_0 / Z_H: l0 holds L_0 on the coset, the division is the closing product below
        // (LINK: z - f_prev(w^rot x_i), the chain relation of a chunked permutation)
        if constexpr (LINK) fr9_load(c, rt.r[qarg.link_row] + 8 * ((i + qarg.link_rot) & (n - 1)));
        else fr9_one(c);
        fr9_sub4(z, z, c);
        fr9_load(c, l0 + 8 * i);
        fr9_mul(t, z, c);
        lds_get(c, cst, QS_ALPHA2);
        fr9_mul(t, t, c);
        fr9_add(acc, acc, t);
        fr9_norm(acc, acc);
    }
    if constexpr (EXT) {
        if (qx.n_lookups) {
            // the running fraction of k_lk_step, point by point and without the inversion: P / Q = sum_l 1 / D_l - m / D_0
            //   P = -m, Q = D_0;  (P, Q) <- (P D_l + Q, Q D_l) for every l;  LK1 = (S(w x) - S(x)) Q - P
            // P is 4r - m (< 5r) at first and (a product) + Q < 2r + 4r afterwards: a first operand below 6r against D_l
            // below 4r.  Q is D_0 and then a product's output: normalised either way.
            fr9_t theta, beta, P, Q, d, s, t;
            lds_get(theta, cst, QX_THETA);
            lds_get(beta, cst, QX_LBETA);
            quot_lk_den(Q, rt, qx.tab_row, qx.width, i, theta, beta);
            fr9_load(c, rt.r[qx.mult_row] + 8 * i);
            fr9_zero(P);
            fr9_sub4(P, P, c);
            for (uint32_t l = 0; l < qx.n_lookups; l++) {
                quot_lk_den(d, rt, qx.in_row + l * qx.width, qx.width, i, theta, beta);
                fr9_mul(P, P, d);
                fr9_add(P, P, Q);
                fr9_mul(Q, Q, d);
            }
            const uint32_t* sr = rt.r[qx.sum_row];
            fr9_load(s, sr + 8 * i);
            fr9_load(t, sr + 8 * ((i + ((uint64_t)1 << qa.ext_log)) & (n - 1)));
            fr9_sub4(t, t, s);                // S(w x) - S(x), < 5r
            fr9_mul(t, t, Q);
            fr9_norm(P, P);                   // < 6r, normalised: what fr9_sub8 takes
            fr9_sub8(t, t, P);                // LK1, < 10r
            if constexpr (ACT) fr9_mul(t, t, act);   // A LK1, < 2r
            lds_get(c, cst, QX_ALPHA3);
            fr9_mul(t, t, c);
            fr9_add(acc, acc, t);
            fr9_norm(acc, acc);
            // LK2 = S L_0
            fr9_load(c, l0 + 8 * i);
            fr9_mul(t, s, c);
            lds_get(c, cst, QX_ALPHA4);
            fr9_mul(t, t, c);
            fr9_add(acc, acc, t);
            fr9_norm(acc, acc);
        }
    }
    fr9_load(c, qc + 8 * (i & ((1u << qa.ext_log) - 1)));
    fr9_mul(acc, acc, c);
    fr9_canon(acc, acc);
    fr9_store(out + 8 * i, acc);
}
// kzg_rows_commit_quotient_sel / kzg_rows_quotient_part_sel: q_l is the numerator of lookup l's fraction.  Inside the LK1 loop
// P <- P D_l + q_l Q instead of P D_l + Q, one more 32-byte load and one more product per SELECTED lookup and point, behind a
// wave-uniform branch on sel_row[l].  q_l(x_i) is a canonical row value and Q is normalised (D_0 below 4r, then products'
// outputs): q_l Q is a product's output below 2r, so P stays below 2r + 2r, inside the 6r the loop already allows.  A KERNEL OF
// ITS OWN with a body of its own (k_quot_points above is the text it was before the selectors existed, so that every existing
// call keeps its instructions), always with the extended argument, in the four <ACT, LINK> combinations the two calls reach.
template <bool ACT, bool LINK>
__global__ void __launch_bounds__(256) k_quot_points_sel(const RowTab rt, const uint32_t* __restrict__ l0,
                                                          uint32_t* __restrict__ out, int log_n, const QuotArgS qarg,
                                                          const uint32_t* __restrict__ tw, const uint32_t* __restrict__ qc,
                                                          uint32_t* __restrict__ bad) {
    constexpr bool EXT = true;   // (the text below is k_quot_points' with the selector in the LK1 loop)
    static_assert(EXT || !ACT, "the active column comes with the extended argument");
    static_assert(EXT || !LINK, "the link comes with the extended argument");
    const auto& qx = quot_ext(qarg);   // (the plain argument itself when !EXT: nothing of it is read through qx then)
    const QuotArg& qa = quot_base(qarg);
    __shared__ uint32_t cst[EXT ? QX_COUNT : QS_COUNT][9];
    const uint32_t v = threadIdx.x;
    const bool chk = blockIdx.x == 0;
    if (v < QS_COUNT) {
        fr9_t c;
        bool live = true;
        if (v < QS_SHIFT) {
            live = v < qa.n_terms;
            if (live) quot_arg(c, qa.c[v], bad, chk);
        } else if (v < QS_BETA) {   // beta s_j
            live = v - QS_SHIFT < qa.k;
            if (live) {
                fr9_t b;
                quot_arg(c, qa.shift[v - QS_SHIFT], bad, chk);
                quot_arg(b, qa.beta, bad, false);
                fr9_mul(c, c, b);
                fr9_canon(c, c);
            }
        } else if (v == QS_BETA) {
            quot_arg(c, qa.beta, bad, chk);
        } else if (v == QS_GAMMA) {
            quot_arg(c, qa.gamma, bad, chk);
        } else {
            quot_arg(c, qa.alpha, bad, chk);
            if (v == QS_ALPHA2) {
                fr9_mul(c, c, c);
                fr9_canon(c, c);
            }
        }
        if (!live) fr9_zero(c);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
    }
    if constexpr (EXT) {
        if (v >= QS_COUNT && v < QX_COUNT) {   // theta, the lookup's beta, alpha^3, alpha^4: one lane each
            fr9_t c;
            if (v == QX_THETA) {
                quot_arg(c, qx.theta, bad, chk);
            } else if (v == QX_LBETA) {
                quot_arg(c, qx.lbeta, bad, chk);
            } else {
                fr9_t a2;
                quot_arg(c, qa.alpha, bad, false);
                fr9_mul(a2, c, c);
                fr9_canon(a2, a2);
                fr9_mul(c, v == QX_ALPHA3 ? c : a2, a2);
                fr9_canon(c, c);
            }
#pragma unroll
            for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
        }
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + v;
    if (i >> log_n) return;
    const uint64_t n = (uint64_t)1 << log_n, half = n >> 1;
    fr9_t acc, p, c;
    [[maybe_unused]] fr9_t act;
    if constexpr (ACT) {
        if (qa.k || qx.n_lookups) fr9_load(act, rt.r[quot_active_row(qarg)] + 8 * i);
    }
    fr9_zero(acc);
    for (uint32_t u = 0; u < qa.n_terms; u++) {
        lds_get(p, cst, u);
        const uint32_t len = qa.len[u];
        for (uint32_t f = 0; f < len; f++) {
            if constexpr (EXT) fr9_load(c, rt.r[qa.row[u][f]] + 8 * ((i + qx.rot[u][f]) & (n - 1)));
            else fr9_load(c, rt.r[qa.row[u][f]] + 8 * i);
            fr9_mul(p, p, c);
        }
        fr9_add(acc, acc, p);
        fr9_norm(acc, acc);
    }
    if (qa.k) {
        fr9_t x, g, gamma, beta, A, B, z, a, sg, t, fa;
        // x_i = g w_N^i, kept lazy (a first operand only)
        fr9_load(g, qc + 8 * QC_G);
        tw_get(c, tw, i & (half - 1));
        fr9_mul(x, g, c);
        if (i >= half) {
            fr9_zero(t);
            fr9_sub4(x, t, x);
        }
        lds_get(gamma, cst, QS_GAMMA);
        lds_get(beta, cst, QS_BETA);
        const uint32_t* zr = rt.r[qa.z_row];
        fr9_load(z, zr + 8 * i);
        fr9_load(B, zr + 8 * ((i + ((uint64_t)1 << qa.ext_log)) & (n - 1)));
        A = z;
        for (uint32_t j = 0; j < qa.k; j++) {
            fr9_load(a, rt.r[qa.wire[j]] + 8 * i);
            fr9_load(sg, rt.r[qa.sigma[j]] + 8 * i);
            lds_get(c, cst, QS_SHIFT + j);
            fr9_mul(t, x, c);                 // beta s_j x_i
            fr9_add(fa, a, gamma);
            fr9_add(t, t, fa);                // < 4r
            fr9_norm(t, t);
            fr9_mul(A, t, A);
            fr9_mul(t, sg, beta);
            fr9_add(t, t, fa);
            fr9_norm(t, t);
            fr9_mul(B, t, B);
        }
        fr9_sub4(A, A, B);                    // P1, < 6r
        if constexpr (ACT) fr9_mul(A, A, act);   // A P1, < 2r
        lds_get(c, cst, QS_ALPHA);
        fr9_mul(t, A, c);
        fr9_add(acc, acc, t);
        fr9_norm(acc, acc);
        // P2 / Z_H = (z - 1) L_0 / Z_H: l0 holds L_0 on the coset, the division is the closing product below
        // (LINK: z - f_prev(w^rot x_i), the chain relation of a chunked permutation)
        if constexpr (LINK) fr9_load(c, rt.r[qarg.l.link_row] + 8 * ((i + qarg.l.link_rot) & (n - 1)));
        else fr9_one(c);
        fr9_sub4(z, z, c);
        fr9_load(c, l0 + 8 * i);
        fr9_mul(t, z, c);
        lds_get(c, cst, QS_ALPHA2);
        fr9_mul(t, t, c);
        fr9_add(acc, acc, t);
        fr9_norm(acc, acc);
    }
    if constexpr (EXT) {
        if (qx.n_lookups) {
            // the running fraction of k_lk_step, point by point and without the inversion: P / Q = sum_l 1 / D_l - m / D_0
            //   P = -m, Q = D_0;  (P, Q) <- (P D_l + Q, Q D_l) for every l;  LK1 = (S(w x) - S(x)) Q - P
            // P is 4r - m (< 5r) at first and (a product) + Q < 2r + 4r afterwards: a first operand below 6r against D_l
            // below 4r.  Q is D_0 and then a product's output: normalised either way.
            fr9_t theta, beta, P, Q, d, s, t;
            lds_get(theta, cst, QX_THETA);
            lds_get(beta, cst, QX_LBETA);
            quot_lk_den(Q, rt, qx.tab_row, qx.width, i, theta, beta);
            fr9_load(c, rt.r[qx.mult_row] + 8 * i);
            fr9_zero(P);
            fr9_sub4(P, P, c);
            for (uint32_t l = 0; l < qx.n_lookups; l++) {
                quot_lk_den(d, rt, qx.in_row + l * qx.width, qx.width, i, theta, beta);
                fr9_mul(P, P, d);
                const uint32_t sr = qarg.sel_row[l];   // wave-uniform: a kernel argument
                if (sr != QUOT_NO_SEL) {
                    fr9_load(c, rt.r[sr] + 8 * i);
                    fr9_mul(t, c, Q);                 // q_l Q, < 2r
                    fr9_add(P, P, t);
                } else {
                    fr9_add(P, P, Q);
                }
                fr9_mul(Q, Q, d);
            }
            const uint32_t* sr = rt.r[qx.sum_row];
            fr9_load(s, sr + 8 * i);
            fr9_load(t, sr + 8 * ((i + ((uint64_t)1 << qa.ext_log)) & (n - 1)));
            fr9_sub4(t, t, s);                // S(w x) - S(x), < 5r
            fr9_mul(t, t, Q);
            fr9_norm(P, P);                   // < 6r, normalised: what fr9_sub8 takes
            fr9_sub8(t, t, P);                // LK1, < 10r
            if constexpr (ACT) fr9_mul(t, t, act);   // A LK1, < 2r
            lds_get(c, cst, QX_ALPHA3);
            fr9_mul(t, t, c);
            fr9_add(acc, acc, t);
            fr9_norm(acc, acc);
            // LK2 = S L_0
            fr9_load(c, l0 + 8 * i);
            fr9_mul(t, s, c);
            lds_get(c, cst, QX_ALPHA4);
            fr9_mul(t, t, c);
            fr9_add(acc, acc, t);
            fr9_norm(acc, acc);
        }
    }
    fr9_load(c, qc + 8 * (i & ((1u << qa.ext_log) - 1)));
    fr9_mul(acc, acc, c);
    fr9_canon(acc, acc);
    fr9_store(out + 8 * i, acc);
}
void launch_quot_points(hipStream_t s, const RowTab& ext_rows, const uint32_t* l0, uint32_t* out, int log_t, const QuotPlan& qp,
                        const uint32_t* tw_n, const uint32_t* qc, uint32_t* bad) {
    QuotArgS sarg;
    QuotArgL& larg = sarg.l;
    QuotArgA& qarg = larg.a;
    QuotArgX& qx = qarg.x;
    QuotArg& qa = qx.q;
    memset(&sarg, 0, sizeof(sarg));
    qa.n_terms = qp.n_terms;
    qa.k = qp.k;
    qa.z_row = qp.z_row;
    qa.ext_log = qp.ext_log;
    for (uint32_t u = 0; u < qp.n_terms; u++) {
        memcpy(qa.c[u].w, qp.term_coeffs_be32 + 32 * (size_t)u, 32);
        qa.len[u] = qp.term_len[u];
        memcpy(qa.row[u], qp.term_row[u], QUOT_MAX_FACTORS);
    }
    for (uint32_t j = 0; j < qp.k; j++) {
        memcpy(qa.shift[j].w, qp.shifts_be32 + 32 * (size_t)j, 32);
        qa.wire[j] = qp.wire[j];
        qa.sigma[j] = qp.sigma[j];
    }
    if (qp.k) {
        memcpy(qa.beta.w, qp.beta_be32, 32);
        memcpy(qa.gamma.w, qp.gamma_be32, 32);
    }
    if (qp.k || qp.n_lookups) memcpy(qa.alpha.w, qp.alpha_be32, 32);
    const int log_n = log_t + (int)qp.ext_log;
    const dim3 g(nblk((uint64_t)1 << log_n, 256));
    if (!qp.ext) {
        k_quot_points<false><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, qa, tw_n, qc, bad);
        return;
    }
    for (uint32_t u = 0; u < qp.n_terms; u++)
        for (uint32_t f = 0; f < qp.term_len[u]; f++) qx.rot[u][f] = qp.term_rot[u][f] << qp.ext_log;
    if (qp.n_lookups) {
        memcpy(qx.theta.w, qp.theta_be32, 32);
        memcpy(qx.lbeta.w, qp.lbeta_be32, 32);
        memcpy(qx.in_row, qp.in_row, sizeof(qx.in_row));
        memcpy(qx.tab_row, qp.tab_row, sizeof(qx.tab_row));
        qx.n_lookups = qp.n_lookups;
        qx.width = qp.width;
        qx.mult_row = qp.mult_row;
        qx.sum_row = qp.sum_row;
    }
    if (qp.active) qarg.active_row = qp.active_row;
    if (qp.link) {
        larg.link_row = qp.link_row;
        larg.link_rot = qp.link_rot << qp.ext_log;
    }
    if (qp.sel) {   // (then n_lookups > 0: the host's check)
        memcpy(sarg.sel_row, qp.sel_row, sizeof(sarg.sel_row));
#define QS_GO(A, L) k_quot_points_sel<A, L><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, sarg, tw_n, qc, bad)
        if (qp.active) { if (qp.link) QS_GO(true, true); else QS_GO(true, false); }
        else { if (qp.link) QS_GO(false, true); else QS_GO(false, false); }
#undef QS_GO
        return;
    }
    if (qp.link) {
        if (qp.active) k_quot_points<true, true, true><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, larg, tw_n, qc, bad);
        else k_quot_points<true, false, true><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, larg, tw_n, qc, bad);
        return;
    }
    if (!qp.active) {
        k_quot_points<true><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, qx, tw_n, qc, bad);
        return;
    }
    k_quot_points<true, true><<<g, 256, 0, s>>>(ext_rows, l0, out, log_n, qarg, tw_n, qc, bad);
}

// ------------------------------------------------------------------------------------------------ the accumulator's add
// acc[i] = scale v[i] (FIRST: the part that creates the accumulator) or acc[i] + scale v[i], canonical on store; v is one part's
// num / Z_H on the coset (canonical), scale the caller's canonical scalar, converted to Montgomery form once per workgroup.  The
// product is below 2r and the sum with a canonical acc[i] below 3r: fr9_reduce takes it.  Streaming: one product per element,
// 64 B in (32 when FIRST), 32 B out.
template <bool FIRST>
__global__ void __launch_bounds__(256) k_quot_accumulate(uint32_t* __restrict__ acc, const uint32_t* __restrict__ v, uint64_t n,
                                                          const FrArg scale) {
    __shared__ uint32_t cst[9];
    if (threadIdx.x == 0) {   // (scale < r is the host's check: the add raises no flag, it is the call's last device step)
        fr9_t c;
        quot_arg(c, scale, nullptr, false);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[i] = c.l[i];
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr9_t sc, p;
#pragma unroll
    for (int k = 0; k < 9; k++) sc.l[k] = cst[k];
    fr9_load(p, v + 8 * i);
    fr9_mul(p, p, sc);
    if constexpr (FIRST) {
        fr9_canon(p, p);
    } else {
        fr9_t o;
        fr9_load(o, acc + 8 * i);
        fr9_add(p, p, o);
        fr9_reduce(p, p);
    }
    fr9_store(acc + 8 * i, p);
}
void launch_quot_accumulate(hipStream_t s, uint32_t* acc, const uint32_t* v, uint64_t n, const uint8_t* scale_be32_or_null,
                            bool first) {
    if (!n) return;
    FrArg sc;
    memset(&sc, 0, sizeof(sc));
    if (scale_be32_or_null) memcpy(sc.w, scale_be32_or_null, 32);
    else reinterpret_cast<uint8_t*>(sc.w)[31] = 1;   // big-endian 1
    if (first) k_quot_accumulate<true><<<nblk(n, 256), 256, 0, s>>>(acc, v, n, sc);
    else k_quot_accumulate<false><<<nblk(n, 256), 256, 0, s>>>(acc, v, n, sc);
}

// ------------------------------------------------------------------------------------------------ back to the pieces
__global__ void __launch_bounds__(256) k_quot_pieces(const uint32_t* __restrict__ in, uint32_t* __restrict__ dst, int log_n,
                                                      uint64_t kept, const uint32_t* __restrict__ qc,
                                                      uint32_t* __restrict__ tail_flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    if (i >= kept) {   // canonical input: zero exactly when every word is
        const uint4* q = reinterpret_cast<const uint4*>(in + 8 * i);
        const uint4 a = q[0], b = q[1];
        if (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) atomicOr(tail_flag, 1u);
        return;
    }
    fr9_t p, c;
    quot_gpow(p, qc, log_n, 1, i);
    fr9_load(c, in + 8 * i);
    fr9_mul(p, p, c);
    fr9_canon(p, p);
    fr9_store(dst + 8 * i, p);
}
void launch_quot_pieces(hipStream_t s, const uint32_t* in, uint32_t* dst, int log_t, int ext_log, uint32_t n_pieces,
                        const uint32_t* qc, uint32_t* tail_flag) {
    const int log_n = log_t + ext_log;
    k_quot_pieces<<<nblk((uint64_t)1 << log_n, 256), 256, 0, s>>>(in, dst, log_n, (uint64_t)n_pieces << log_t, qc, tail_flag);
}
