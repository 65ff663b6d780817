// fr_lookup.hip -- Fr-side kernels, part 5: the lookup (logUp) running sum of kzg_rows_commit_lookup_sum.  A running
// FRACTION per domain point over transformed rows, the library's batched inversion (the prefix / suffix product scan of
// fr_prod.hip over ONE vector and its one fr9_inv) and a chunked multi-level additive prefix scan (the shape of fr_prod.hip's
// scan with the monoid "add").
//   F_l = sum_c theta^c f_{l,c},  Tb = sum_c theta^c t_c                      (Horner in c, one column at a time)
//   P_t / Q_t = sum_l 1 / (beta + F_l(w^t)) - m(w^t) / (beta + Tb(w^t))       (P, Q: two running vectors)
//   1 / Q_t = (prod_{u<t} Q_u) (prod_{u>t} Q_u) (prod_u Q_u)^-1               -- ONE inversion per call
//   S(w^t) = sum_{u<t} P_u / Q_u,  closing = sum_u P_u / Q_u
// Running values stay in the product's output class or the lazy class and are canonicalised on store (fr29.hip.h).
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// ------------------------------------------------------------------------------------------------ the running fraction
// One transformed column e (n evaluations, Montgomery, natural order) enters the call.  v = acc theta + e (e alone when the
// column is the first of its Horner chain: HAS_ACC false), then
//   LK_HORNER : acc <- v                                     (more columns of this tuple follow)
//   LK_TABLE  : Q <- beta + v,  P <- -P                      (P holds m's evaluations: the fraction starts as -m / d_T)
//   LK_INPUT  : (P, Q) <- (P d + Q, Q d) with d = beta + v   (one more 1 / d)
//   LK_INPUT_SEL : (P, Q) <- (P d + q Q, Q d)                (one more q / d: kzg_rows_commit_lookup_sum_sel, q the
//                  lookup's selector row in evaluation form, any element of Fr)
// theta and beta are converted to Montgomery form once per workgroup (two lanes, one product each).  Multiplier-bound at
// LK_INPUT (2 or 3 products per element, 96 - 128 B in, 64 B out), bandwidth-bound otherwise (0 or 1 product).
// LK_INPUT_SEL does 3 or 4 products per element and reads 32 B more (q).  Operand classes: p, q and the selector are loaded
// canonical (the forward transform ends in fr9_reduce, P and Q are stored canonical), d is normalised below 4r: p d and q Q
// are both products' outputs below 2r, so their sum is below 4r with limbs < 2^30, inside what fr9_reduce takes.  The mode
// is a kernel of its own, k_lk_step_sel, with an argument struct of its own (the selector's pointer rides there), so the three
// other modes keep their signature, their names and their instructions; a lookup without a selector still launches LK_INPUT.
enum { LK_HORNER = 0, LK_TABLE = 1, LK_INPUT = 2, LK_INPUT_SEL = 3 };
struct LkArg {
    FrArg theta, beta;
};
struct LkArgSel {
    LkArg a;
    const uint32_t* sel;
};
KZG_DEV void lk_from_arg(fr9_t& v, const FrArg& a, uint32_t* __restrict__ bad, bool check) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(a.w[7 - i]);
    if (check && fr_words_ge_r(w)) atomicOr(bad, 1u);
    fr9_from_words(v, w);
    fr9_to_mont(v, v);
}
template <int MODE, bool HAS_ACC>
__global__ void __launch_bounds__(256) k_lk_step(const uint32_t* __restrict__ e, uint32_t* __restrict__ acc,
                                                  uint32_t* __restrict__ P, uint32_t* __restrict__ Q, uint64_t n,
                                                  const LkArg arg, uint32_t* __restrict__ bad) {
    __shared__ uint32_t cst[2][9];   // theta, beta
    const uint32_t lane = threadIdx.x;
    if (lane < 2) {
        fr9_t c;
        lk_from_arg(c, lane ? arg.beta : arg.theta, bad, blockIdx.x == 0);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[lane][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + lane;
    if (t >= n) return;
    fr9_t v, x;
    fr9_load(v, e + 8 * t);
    if constexpr (HAS_ACC) {
        fr9_t a, theta;
#pragma unroll
        for (int i = 0; i < 9; i++) theta.l[i] = cst[0][i];
        fr9_load(a, acc + 8 * t);
        fr9_mul(x, a, theta);
        fr9_add(v, v, x);                     // < 3r, limbs < 2^30
    }
    if constexpr (MODE == LK_HORNER) {
        fr9_reduce(v, v);
        fr9_store(acc + 8 * t, v);
        return;
    }
    fr9_t beta, d, p, q;
#pragma unroll
    for (int i = 0; i < 9; i++) beta.l[i] = cst[1][i];
    fr9_add(d, v, beta);                      // < 4r, limbs < 2^31
    fr9_load(p, P + 8 * t);
    if constexpr (MODE == LK_TABLE) {
        fr9_reduce(d, d);
        fr9_zero(x);
        fr9_sub4(x, x, p);                    // 4r - m
        fr9_reduce(x, x);
        fr9_store(Q + 8 * t, d);
        fr9_store(P + 8 * t, x);
    } else {
        fr9_norm(d, d);                       // a legal second operand: limbs 0..7 < 2^29, value < 4r
        fr9_load(q, Q + 8 * t);
        fr9_mul(x, p, d);
        fr9_add(x, x, q);                     // < 3r
        fr9_reduce(x, x);
        fr9_mul(q, q, d);
        fr9_canon(q, q);
        fr9_store(P + 8 * t, x);
        fr9_store(Q + 8 * t, q);
    }
}
void launch_lk_step(hipStream_t s, const uint32_t* e, uint32_t* acc, uint32_t* P, uint32_t* Q, uint64_t n, int mode,
                    bool has_acc, const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint32_t* bad) {
    if (!n) return;
    LkArg arg;
    memcpy(arg.theta.w, theta_be32, 32);
    memcpy(arg.beta.w, beta_be32, 32);
    const dim3 g(nblk(n, 256));
#define LK_GO(M, H) k_lk_step<M, H><<<g, 256, 0, s>>>(e, acc, P, Q, n, arg, bad)
    if (mode == LK_HORNER) { if (has_acc) LK_GO(LK_HORNER, true); else LK_GO(LK_HORNER, false); }
    else if (mode == LK_TABLE) { if (has_acc) LK_GO(LK_TABLE, true); else LK_GO(LK_TABLE, false); }
    else { if (has_acc) LK_GO(LK_INPUT, true); else LK_GO(LK_INPUT, false); }
#undef LK_GO
}

// LK_INPUT_SEL: the LK_INPUT step with the numerator q = sel[t].  A kernel of its own (k_lk_step keeps its signature, its names
// and its instructions); the front is k_lk_step's.
template <bool HAS_ACC>
__global__ void __launch_bounds__(256) k_lk_step_sel(const uint32_t* __restrict__ e, uint32_t* __restrict__ acc,
                                                      uint32_t* __restrict__ P, uint32_t* __restrict__ Q, uint64_t n,
                                                      const LkArgSel larg, uint32_t* __restrict__ bad) {
    __shared__ uint32_t cst[2][9];   // theta, beta
    const uint32_t lane = threadIdx.x;
    if (lane < 2) {
        fr9_t c;
        lk_from_arg(c, lane ? larg.a.beta : larg.a.theta, bad, blockIdx.x == 0);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[lane][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + lane;
    if (t >= n) return;
    fr9_t v, x, y, beta, d, p, q, s;
    fr9_load(v, e + 8 * t);
    if constexpr (HAS_ACC) {
        fr9_t a, theta;
#pragma unroll
        for (int i = 0; i < 9; i++) theta.l[i] = cst[0][i];
        fr9_load(a, acc + 8 * t);
        fr9_mul(x, a, theta);
        fr9_add(v, v, x);                     // < 3r, limbs < 2^30
    }
#pragma unroll
    for (int i = 0; i < 9; i++) beta.l[i] = cst[1][i];
    fr9_add(d, v, beta);                      // < 4r, limbs < 2^31
    fr9_norm(d, d);                           // a legal second operand: limbs 0..7 < 2^29, value < 4r
    fr9_load(p, P + 8 * t);
    fr9_load(q, Q + 8 * t);
    fr9_load(s, larg.sel + 8 * t);            // q_l(w^t), canonical
    fr9_mul(x, p, d);
    fr9_mul(y, s, q);
    fr9_add(x, x, y);                         // < 4r, limbs < 2^30
    fr9_reduce(x, x);
    fr9_mul(q, q, d);
    fr9_canon(q, q);
    fr9_store(P + 8 * t, x);
    fr9_store(Q + 8 * t, q);
}
void launch_lk_step_sel(hipStream_t s, const uint32_t* e, uint32_t* acc, uint32_t* P, uint32_t* Q, const uint32_t* sel,
                        uint64_t n, bool has_acc, const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint32_t* bad) {
    if (!n) return;
    LkArgSel arg;
    memcpy(arg.a.theta.w, theta_be32, 32);
    memcpy(arg.a.beta.w, beta_be32, 32);
    arg.sel = sel;
    const dim3 g(nblk(n, 256));
    if (has_acc) k_lk_step_sel<true><<<g, 256, 0, s>>>(e, acc, P, Q, n, arg, bad);
    else k_lk_step_sel<false><<<g, 256, 0, s>>>(e, acc, P, Q, n, arg, bad);
}

// ------------------------------------------------------------------------------------------------ batched inversion
// Level 0 of the inversion, chunk g of 2^l elements, behind launch_gp_scan_upper(Q, Q): exN[g] is the product of every Q in
// front of the chunk, exD[g] the product of every Q behind it times 1 / prod Q.  Downward, W[t] <- the exclusive suffix
// product behind t (carrying the inverse); upward, 1 / Q_t = (exclusive prefix at t) * W[t], and out[t] <- P[t] / Q_t
// (HAS_P) or 1 / Q_t.  3 or 4 products per element; multiplier-bound.  out may be P or W (a lane reads t before it writes t).
template <bool HAS_P>
__global__ void __launch_bounds__(256) k_lk_inv_final(const uint32_t* __restrict__ Q, uint32_t* W, const uint32_t* P,
                                                       uint32_t* out, uint64_t n, int l, const uint32_t* __restrict__ exN,
                                                       const uint32_t* __restrict__ exD) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t p, c, o;
    fr9_load(p, exD + 8 * g);
    for (uint64_t t = hi; t-- > lo;) {
        fr9_load(c, Q + 8 * t);
        fr9_canon(o, p);
        fr9_store(W + 8 * t, o);
        fr9_mul(p, p, c);
    }
    fr9_load(p, exN + 8 * g);
    for (uint64_t t = lo; t < hi; t++) {
        fr9_t inv;
        fr9_load(c, W + 8 * t);           // this lane's own store above
        fr9_mul(inv, p, c);
        if constexpr (HAS_P) {
            fr9_load(c, P + 8 * t);
            fr9_mul(inv, c, inv);
        }
        fr9_canon(inv, inv);
        fr9_store(out + 8 * t, inv);
        fr9_load(c, Q + 8 * t);
        fr9_mul(p, p, c);
    }
}
void launch_fr_batch_inv(hipStream_t s, const ScanPlan& pl, const uint32_t* Q, uint32_t* W, const uint32_t* P_or_null,
                         uint32_t* out, uint64_t n, uint32_t* scrN, uint32_t* scrD, uint8_t* scratch32, uint32_t* zero_flag) {
    const int l0 = launch_gp_scan_upper(s, pl, Q, Q, n, scrN, scrD, scratch32, zero_flag);
    if (l0 < 0) return;
    const uint32_t blocks = nblk(pl.n[1], 256);
    if (P_or_null) k_lk_inv_final<true><<<blocks, 256, 0, s>>>(Q, W, P_or_null, out, n, l0, scrN, scrD);
    else k_lk_inv_final<false><<<blocks, 256, 0, s>>>(Q, W, nullptr, out, n, l0, scrN, scrD);
}
void launch_fr_batch_inv(hipStream_t s, const uint32_t* Q, uint32_t* W, const uint32_t* P_or_null, uint32_t* out, uint64_t n,
                         uint32_t* scrN, uint32_t* scrD, uint8_t* scratch32, uint32_t* zero_flag) {
    if (n) launch_fr_batch_inv(s, scan_plan(n), Q, W, P_or_null, out, n, scrN, scrD, scratch32, zero_flag);
}

// ------------------------------------------------------------------------------------------------ additive scan
// a + b mod r of two canonical values, canonical
KZG_DEV void fr9_addmod(fr9_t& r, const fr9_t& a, const fr9_t& b) {
    fr9_t t;
    fr9_add(t, a, b);
    fr9_norm(t, t);
    fr9_canon(r, t);
}
// Level k + 1 holds the sums of 2^l consecutive values of level k.  Bandwidth-bound (no product).
__global__ void __launch_bounds__(256) k_lk_chunk_sum(const uint32_t* __restrict__ in, uint64_t n, int l,
                                                       uint32_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t p, c;
    fr9_load(p, in + 8 * lo);
    for (uint64_t u = lo + 1; u < hi; u++) {
        fr9_load(c, in + 8 * u);
        fr9_addmod(p, p, c);
    }
    fr9_store(out + 8 * g, p);
}
// The top level (m <= LK_TOP_MAX values), one workgroup: the values become their EXCLUSIVE PREFIX sums in place (a lane folds
// its <= 8 consecutive values, a Hillis-Steele scan over the 256 lane sums gives each lane its start); the total -- the
// closing value -- goes to the record as 32 big-endian bytes.
#define LK_TOP_MAX 2048
__global__ void __launch_bounds__(256) k_lk_top_sum(uint32_t* __restrict__ vals, uint32_t m, uint8_t* __restrict__ closing_be) {
    __shared__ uint32_t sm[9][256];
    const uint32_t v = threadIdx.x;
    const uint32_t per = (m + 255u) / 256u;
    const uint32_t lo = v * per, hi = lo + per < m ? lo + per : m;
    fr9_t g, c;
    fr9_zero(g);
    for (uint32_t u = lo; u < hi; u++) {
        fr9_load(c, vals + 8 * (uint64_t)u);
        fr9_addmod(g, g, c);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) sm[i][v] = g.l[i];
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        fr9_t other;
        const bool has = v >= d;
        if (has) {
#pragma unroll
            for (int i = 0; i < 9; i++) other.l[i] = sm[i][v - d];
        }
        __syncthreads();
        if (has) {
            fr9_addmod(g, g, other);
#pragma unroll
            for (int i = 0; i < 9; i++) sm[i][v] = g.l[i];
        }
        __syncthreads();
    }
    // sm[.][v] = sum of the values of lanes 0 .. v; lane 255's is the total
    if (v == 255) {
        fr9_t cl;
        fr9_from_mont(cl, g);
        uint32_t w[8];
        fr9_to_words(w, cl);
        limbs_to_be<8>(closing_be, w);
    }
    fr9_t p;
    if (v) {
#pragma unroll
        for (int i = 0; i < 9; i++) p.l[i] = sm[i][v - 1];
    } else {
        fr9_zero(p);
    }
    for (uint32_t u = lo; u < hi; u++) {
        fr9_load(c, vals + 8 * (uint64_t)u);
        fr9_store(vals + 8 * (uint64_t)u, p);
        fr9_addmod(p, p, c);
    }
}
// One level down, in place: group g of 2^l values of this level starts from the parent's exclusive value ex[g]; each value is
// replaced by the exclusive sum in front of it.  At level 0 that is S itself.
__global__ void __launch_bounds__(256) k_lk_expand_sum(uint32_t* __restrict__ vals, uint64_t n, int l,
                                                        const uint32_t* __restrict__ ex) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t p, c;
    fr9_load(p, ex + 8 * g);
    for (uint64_t u = lo; u < hi; u++) {
        fr9_load(c, vals + 8 * u);
        fr9_store(vals + 8 * u, p);
        fr9_addmod(p, p, c);
    }
}
// The levels of launch_gp_scan_upper, by the same plan (scan_plan, fr_prod.hip): 2^l[0] elements per lane at level 0 (4 for
// short rows, 16 for long ones), 16 above, until at most LK_TOP_MAX values are left.
void launch_lk_sum_scan(hipStream_t s, const ScanPlan& pl, uint32_t* v, uint64_t n, uint32_t* scr, uint8_t* closing_be) {
    if (!scan_plan_runs(pl, n)) return;
    const int K = pl.K;
    for (int k = 0; k < K; k++)
        k_lk_chunk_sum<<<nblk(pl.n[k + 1], 256), 256, 0, s>>>(k ? scr + 8 * pl.off[k] : v, pl.n[k], pl.l[k], scr + 8 * pl.off[k + 1]);
    k_lk_top_sum<<<1, 256, 0, s>>>(scr + 8 * pl.off[K], (uint32_t)pl.n[K], closing_be);
    for (int k = K - 1; k >= 0; k--)
        k_lk_expand_sum<<<nblk(pl.n[k + 1], 256), 256, 0, s>>>(k ? scr + 8 * pl.off[k] : v, pl.n[k], pl.l[k], scr + 8 * pl.off[k + 1]);
}
void launch_lk_sum_scan(hipStream_t s, uint32_t* v, uint64_t n, uint32_t* scr, uint8_t* closing_be) {
    if (n) launch_lk_sum_scan(s, scan_plan(n), v, n, scr, closing_be);
}
