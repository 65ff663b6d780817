// fr_prod.hip -- Fr-side kernels, part 3: the permutation grand product of kzg_rows_commit_grand_product.  Element-wise
// products over transformed rows, a chunked multi-level prefix / suffix PRODUCT scan (the shape of fr_poly.hip's Horner scan
// with the monoid "multiply") and the library's one device-side Fr inversion.
//   N_t = prod_j (a_j(w^t) + beta s_j w^t + gamma),  D_t = prod_j (a_j(w^t) + beta sigma_j(w^t) + gamma)
//   z(w^t) = (prod_{u<t} N_u) (prod_{u>=t} D_u) (prod_u D_u)^-1        -- ONE inversion per call, no batch inversion
// kzg_rows_commit_shuffle feeds the same scans: its N and D come from k_sh_factor (one group and side per launch) instead.
// Every kernel is a chain of fr9_mul: running values stay in the product's output class and are canonicalised on store.
#include <cstring>

#include "fr_inv.hip.h"
#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// ------------------------------------------------------------------------------------------------ inversion
// (fr9_inv: fr_inv.hip.h)
// test hook (kzg_test_field, Fr ops 7 / 8): out[j] = in[j]^-1, or the zero flag of that inversion, as 32 big-endian bytes
__global__ void __launch_bounds__(64) k_fr_inv_test(const uint8_t* __restrict__ in_be, uint8_t* __restrict__ out_be,
                                                    uint64_t n, int want_flag) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t w[8];
    limbs_from_be<8>(w, in_be + 32 * j);
    fr9_t a, y;
    fr9_from_words(a, w);
    fr9_to_mont(a, a);
    const bool ok = fr9_inv(y, a);
    fr9_from_mont(y, y);
    fr9_to_words(w, y);
    if (want_flag) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0;
        w[0] = ok ? 0u : 1u;
    }
    limbs_to_be<8>(out_be + 32 * j, w);
}
void launch_fr_inv_test(hipStream_t s, const uint8_t* in_be, uint8_t* out_be, uint64_t n, int want_flag) {
    if (n) k_fr_inv_test<<<nblk(n, 64), 64, 0, s>>>(in_be, out_be, n, want_flag);
}

// ------------------------------------------------------------------------------------------------ factors
// One wire / sigma pair: N[t] (*)= a(w^t) + beta s w^t + gamma, D[t] (*)= a(w^t) + beta sigma(w^t) + gamma, with ea / es the
// pair's evaluations (forward NTT, natural order) and w^t from the resident forward twiddle table (w^(t + n/2) = -w^t).
// beta, gamma and beta * s are converted to Montgomery form once per workgroup (three lanes, one or two products each).
// FIRST: the vectors are written, not multiplied.  Multiplier-bound: 4 products per element (2 when FIRST), 128 B in, 64 out.
struct GpArg {
    FrArg beta, gamma, shift;
};
KZG_DEV void fr9_from_arg(fr9_t& v, const FrArg& a, uint32_t* __restrict__ bad, bool check) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(a.w[7 - i]);
    if (check && fr_words_ge_r(w)) atomicOr(bad, 1u);
    fr9_from_words(v, w);
    fr9_to_mont(v, v);
}
template <bool FIRST>
__global__ void __launch_bounds__(256) k_gp_factors(const uint32_t* __restrict__ ea, const uint32_t* __restrict__ es,
                                                     uint32_t* __restrict__ N, uint32_t* __restrict__ D, uint64_t n,
                                                     const uint32_t* __restrict__ tw, const GpArg arg,
                                                     uint32_t* __restrict__ bad) {
    __shared__ uint32_t cst[3][9];   // beta, gamma, beta * s
    const uint32_t v = threadIdx.x;
    if (v < 3) {
        fr9_t c;
        fr9_from_arg(c, v == 1 ? arg.gamma : arg.beta, bad, blockIdx.x == 0);
        if (v == 2) {
            fr9_t s;
            fr9_from_arg(s, arg.shift, bad, blockIdx.x == 0);
            fr9_mul(c, c, s);
            fr9_canon(c, c);
        }
#pragma unroll
        for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + v;
    if (t >= n) return;
    fr9_t beta, gamma, bs, a, sg, w, x, fn, fd;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        beta.l[i] = cst[0][i];
        gamma.l[i] = cst[1][i];
        bs.l[i] = cst[2][i];
    }
    fr9_load(a, ea + 8 * t);
    fr9_load(sg, es + 8 * t);
    const uint64_t half = n >> 1;
    if (half) {
        const uint64_t k = t & (half - 1);
        const uint4* q = reinterpret_cast<const uint4*>(tw + 12 * k);
        const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
        w.l[0] = q0.x; w.l[1] = q0.y; w.l[2] = q0.z; w.l[3] = q0.w;
        w.l[4] = q1.x; w.l[5] = q1.y; w.l[6] = q1.z; w.l[7] = q1.w;
        w.l[8] = q2.x;
        fr9_mul(x, bs, w);                    // beta s w^(t mod n/2), < 2r
        if (t >= half) {                      // w^t = -w^(t - n/2)
            fr9_t z;
            fr9_zero(z);
            fr9_sub4(x, z, x);                // 4r - x
        }
    } else {
        x = bs;                               // n == 1: w^0 = 1
    }
    fr9_add(fn, a, gamma);
    fr9_add(fn, fn, x);                       // < 6r, limbs < 2^31
    fr9_norm(fn, fn);
    fr9_mul(x, sg, beta);
    fr9_add(fd, a, gamma);
    fr9_add(fd, fd, x);
    fr9_norm(fd, fd);
    if constexpr (FIRST) {
        fr9_reduce(fn, fn);
        fr9_reduce(fd, fd);
    } else {
        fr9_t o;
        fr9_load(o, N + 8 * t);
        fr9_mul(fn, fn, o);
        fr9_canon(fn, fn);
        fr9_load(o, D + 8 * t);
        fr9_mul(fd, fd, o);
        fr9_canon(fd, fd);
    }
    fr9_store(N + 8 * t, fn);
    fr9_store(D + 8 * t, fd);
}
void launch_gp_factors(hipStream_t s, const uint32_t* ea, const uint32_t* es, uint32_t* N, uint32_t* D, uint64_t n,
                       const uint32_t* tw, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                       const uint8_t shift_be32[32], bool first, uint32_t* bad) {
    if (!n) return;
    GpArg arg;
    memcpy(arg.beta.w, beta_be32, 32);
    memcpy(arg.gamma.w, gamma_be32, 32);
    memcpy(arg.shift.w, shift_be32, 32);
    if (first) k_gp_factors<true><<<nblk(n, 256), 256, 0, s>>>(ea, es, N, D, n, tw, arg, bad);
    else k_gp_factors<false><<<nblk(n, 256), 256, 0, s>>>(ea, es, N, D, n, tw, arg, bad);
}

// ------------------------------------------------------------------------------------------------ shuffle factors
// kzg_rows_commit_shuffle: one side of one group closes its Horner chain in theta and enters its running vector V (N for the
// input side, D for the shuffle side).  e holds the group's column 0 (n evaluations, Montgomery, natural order), acc the chain
// over the columns behind it (HAS_ACC; those steps are fr_lookup.hip's LK_HORNER).  With v = acc theta + e, or e alone:
//   V[t] (*)= gamma + v                         (no selector)
//   V[t] (*)= 1 + q[t] (gamma + v - 1)          (HAS_SEL: q the side's selector row in evaluation form, ANY element of Fr)
// theta and gamma (gamma - 1 under HAS_SEL) are converted to Montgomery form once per workgroup (two lanes).  FIRST: the
// vector is written, not multiplied.  Multiplier-bound: one product each for HAS_ACC, HAS_SEL and !FIRST, so 0 .. 3 per
// element, 32 - 128 B in, 32 B out.  Operand classes: e, acc, q and V are loaded canonical; acc theta is a product's output
// below 2r, so gamma + v stays below 4r with limbs < 2^31, a legal FIRST operand; q (gamma + v - 1) + 1 is below 3r.
struct ShArg {
    FrArg theta, gamma;
    const uint32_t* sel;
};
template <bool FIRST, bool HAS_ACC, bool HAS_SEL>
__global__ void __launch_bounds__(256) k_sh_factor(const uint32_t* __restrict__ e, const uint32_t* __restrict__ acc,
                                                    uint32_t* __restrict__ V, uint64_t n, const ShArg arg,
                                                    uint32_t* __restrict__ bad) {
    __shared__ uint32_t cst[2][9];   // theta, gamma (HAS_SEL: gamma - 1)
    const uint32_t lane = threadIdx.x;
    if (lane < 2) {
        fr9_t c;
        fr9_from_arg(c, lane ? arg.gamma : arg.theta, bad, blockIdx.x == 0);
        if (HAS_SEL && lane) {
            fr9_t one;
            fr9_one(one);
            fr9_sub4(c, c, one);              // gamma + 4r - 1
            fr9_reduce(c, c);
        }
#pragma unroll
        for (int i = 0; i < 9; i++) cst[lane][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + lane;
    if (t >= n) return;
    fr9_t v, x, g;
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
    for (int i = 0; i < 9; i++) g.l[i] = cst[1][i];
    fr9_add(v, v, g);                         // < 4r, limbs < 2^31
    if constexpr (HAS_SEL) {
        fr9_t q;
        fr9_load(q, arg.sel + 8 * t);         // canonical
        fr9_mul(x, v, q);
        fr9_one(g);
        fr9_add(v, x, g);                     // < 3r, limbs < 2^30
    }
    if constexpr (FIRST) {
        fr9_reduce(v, v);
    } else {
        fr9_t o;
        fr9_load(o, V + 8 * t);
        fr9_mul(v, v, o);
        fr9_canon(v, v);
    }
    fr9_store(V + 8 * t, v);
}
void launch_sh_factor(hipStream_t s, const uint32_t* e, const uint32_t* acc_or_null, uint32_t* V, const uint32_t* sel_or_null,
                      uint64_t n, const uint8_t theta_be32[32], const uint8_t gamma_be32[32], bool first, uint32_t* bad) {
    if (!n) return;
    ShArg arg;
    memcpy(arg.theta.w, theta_be32, 32);
    memcpy(arg.gamma.w, gamma_be32, 32);
    arg.sel = sel_or_null;
    const dim3 g(nblk(n, 256));
#define SH_GO(F, A, S) k_sh_factor<F, A, S><<<g, 256, 0, s>>>(e, acc_or_null, V, n, arg, bad)
#define SH_SEL(F, A) do { if (sel_or_null) SH_GO(F, A, true); else SH_GO(F, A, false); } while (0)
    if (first) { if (acc_or_null) SH_SEL(true, true); else SH_SEL(true, false); }
    else { if (acc_or_null) SH_SEL(false, true); else SH_SEL(false, false); }
#undef SH_SEL
#undef SH_GO
}

// ------------------------------------------------------------------------------------------------ product scans
// Level k + 1 holds the products of 2^l consecutive values of level k, for N (grid row 0) and D (grid row 1) side by side.
__global__ void __launch_bounds__(256) k_gp_chunk_prod(const uint32_t* __restrict__ inN, const uint32_t* __restrict__ inD,
                                                        uint64_t n, int lchunk, uint32_t* __restrict__ outN,
                                                        uint32_t* __restrict__ outD) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << lchunk, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    const uint32_t* in = blockIdx.y ? inD : inN;
    fr9_t p, c;
    fr9_load(p, in + 8 * lo);
    for (uint64_t u = lo + 1; u < hi; u++) {
        fr9_load(c, in + 8 * u);
        fr9_mul(p, p, c);
    }
    fr9_canon(p, p);   // (a lone value is canonical already: fr9_canon keeps it)
    fr9_store((blockIdx.y ? outD : outN) + 8 * g, p);
}
// The top level (m <= GP_TOP_MAX values each), one workgroup: lanes [0, 256) turn vN into its EXCLUSIVE PREFIX products,
// lanes [256, 512) turn vD into its EXCLUSIVE SUFFIX products (the same code on the mirrored index), in place: a lane folds
// its <= 8 consecutive values, a Hillis-Steele scan over the 256 lane products gives each lane its start.  Between the scan
// and the walk one lane inverts the total of D (fr9_inv) and every suffix start is multiplied by that inverse, so that
// every value expanded from this level carries it.  The record receives closing = total N / total D (32 bytes big-endian)
// and the zero-denominator flag word.
#define GP_TOP_MAX 2048
__global__ void __launch_bounds__(512) k_gp_top(uint32_t* __restrict__ vN, uint32_t* __restrict__ vD, uint32_t m,
                                                 uint8_t* __restrict__ closing_be, uint32_t* __restrict__ zero_flag) {
    __shared__ uint32_t sm[2][9][256];
    __shared__ uint32_t inv_sm[9];
    const uint32_t side = threadIdx.x >> 8, v = threadIdx.x & 255u;
    uint32_t* vals = side ? vD : vN;
    const uint32_t per = (m + 255u) / 256u;
    const uint32_t lo = v * per, hi = lo + per < m ? lo + per : m;
    auto at = [&](uint32_t u) { return 8 * (uint64_t)(side ? m - 1 - u : u); };
    fr9_t g, c;
    fr9_one(g);
    for (uint32_t u = lo; u < hi; u++) {
        fr9_load(c, vals + at(u));
        fr9_mul(g, g, c);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) sm[side][i][v] = g.l[i];
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {   // products of two N-class values (< 2r each) are legal: 4 r^2 < 2^261 r
        fr9_t other;
        const bool has = v >= d;
        if (has) {
#pragma unroll
            for (int i = 0; i < 9; i++) other.l[i] = sm[side][i][v - d];
        }
        __syncthreads();
        if (has) {
            fr9_mul(g, g, other);
#pragma unroll
            for (int i = 0; i < 9; i++) sm[side][i][v] = g.l[i];
        }
        __syncthreads();
    }
    // sm[side][.][v] = product of the values of lanes 0 .. v; lane 255's is the total
    if (threadIdx.x == 256) {
        fr9_t tot, inv, totn, cl;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            tot.l[i] = sm[1][i][255];
            totn.l[i] = sm[0][i][255];
        }
        const bool ok = fr9_inv(inv, tot);
        *zero_flag = ok ? 0u : 1u;
#pragma unroll
        for (int i = 0; i < 9; i++) inv_sm[i] = inv.l[i];
        fr9_mul(cl, totn, inv);
        fr9_from_mont(cl, cl);
        uint32_t w[8];
        fr9_to_words(w, cl);
        limbs_to_be<8>(closing_be, w);
    }
    __syncthreads();
    fr9_t p;
    if (v) {
#pragma unroll
        for (int i = 0; i < 9; i++) p.l[i] = sm[side][i][v - 1];
    } else {
        fr9_one(p);
    }
    if (side) {
        fr9_t inv;
#pragma unroll
        for (int i = 0; i < 9; i++) inv.l[i] = inv_sm[i];
        fr9_mul(p, p, inv);
    }
    for (uint32_t u = lo; u < hi; u++) {
        fr9_t o;
        fr9_load(c, vals + at(u));
        fr9_canon(o, p);
        fr9_store(vals + at(u), o);
        fr9_mul(p, p, c);
    }
}
// kzg_rows_commit_grand_product_chain: between k_gp_top and the expansions, every EXCLUSIVE PREFIX value of the top level (m <=
// GP_TOP_MAX of them, canonical) is multiplied by the caller's start value, so that every value expanded from this level
// carries it, and lane 0 multiplies the closing value in the record by it as well.  start is converted to Montgomery form once
// per workgroup; a canonical value by a canonical one, canonical on store.  At most 8 workgroups: no pass over the row.
__global__ void __launch_bounds__(256) k_gp_chain_start(uint32_t* __restrict__ vN, uint32_t m, uint8_t* __restrict__ closing_be,
                                                         const FrArg start) {
    __shared__ uint32_t cst[9];
    if (threadIdx.x == 0) {
        fr9_t c;
        fr9_from_arg(c, start, nullptr, false);   // (start < r and != 0 is the host's check)
#pragma unroll
        for (int i = 0; i < 9; i++) cst[i] = c.l[i];
    }
    __syncthreads();
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= m) return;
    fr9_t st, p;
#pragma unroll
    for (int i = 0; i < 9; i++) st.l[i] = cst[i];
    fr9_load(p, vN + 8 * (uint64_t)u);
    fr9_mul(p, p, st);
    fr9_canon(p, p);
    fr9_store(vN + 8 * (uint64_t)u, p);
    if (u == 0) {
        uint32_t w[8];
        limbs_from_be<8>(w, closing_be);
        fr9_from_words(p, w);
        fr9_mul(p, p, st);       // canonical (plain) by Montgomery start: the plain product, below 2r
        fr9_canon(p, p);
        fr9_to_words(w, p);
        limbs_to_be<8>(closing_be, w);
    }
}
// One level down, in place: group g of 2^l values of this level starts from the parent's exclusive value ex[g]; N (grid row
// 0) walks its group upward, D (grid row 1) downward, each value replaced by the exclusive product in front of it.
__global__ void __launch_bounds__(256) k_gp_expand(uint32_t* __restrict__ vN, uint32_t* __restrict__ vD, uint64_t n, int l,
                                                    const uint32_t* __restrict__ exN, const uint32_t* __restrict__ exD) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    const bool down = blockIdx.y != 0;
    uint32_t* vals = down ? vD : vN;
    fr9_t p, c, o;
    fr9_load(p, (down ? exD : exN) + 8 * g);
    for (uint64_t k = 0; k < hi - lo; k++) {
        const uint64_t u = down ? hi - 1 - k : lo + k;
        fr9_load(c, vals + 8 * u);
        fr9_canon(o, p);
        fr9_store(vals + 8 * u, o);
        fr9_mul(p, p, c);
    }
}
// Level 0: chunk g of 2^l elements.  Downward, D[t] becomes the INCLUSIVE suffix product from t (times the inverse of the
// total, carried by exD); upward, z(w^t) = (exclusive prefix of N at t) * D[t] replaces N[t].  3 products per element.
__global__ void __launch_bounds__(256) k_gp_final(uint32_t* __restrict__ N, uint32_t* __restrict__ D, uint64_t n, int l,
                                                   const uint32_t* __restrict__ exN, const uint32_t* __restrict__ exD) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t p, c, o;
    fr9_load(p, exD + 8 * g);
    for (uint64_t t = hi; t-- > lo;) {
        fr9_load(c, D + 8 * t);
        fr9_mul(p, p, c);
        fr9_canon(o, p);
        fr9_store(D + 8 * t, o);
    }
    fr9_load(p, exN + 8 * g);
    for (uint64_t t = lo; t < hi; t++) {
        fr9_t z;
        fr9_load(c, D + 8 * t);       // this lane's own store above
        fr9_mul(z, p, c);
        fr9_canon(z, z);
        fr9_load(c, N + 8 * t);
        fr9_store(N + 8 * t, z);
        fr9_mul(p, p, c);
    }
}
// ---- the plan: pure host arithmetic (fr_kernels.hip.h), shared with the additive scan of fr_lookup.hip.  The level loop is the
// recurrence scan's (ladder_plan_levels) with at least one level under the top
ScanPlan scan_plan_levels(uint64_t n, int l0, uint64_t top_max) { return ladder_plan_levels(n, l0, top_max, 1); }
ScanPlan scan_plan(uint64_t n) {
    int l0 = 2;
    while (l0 < 4 && (n >> (l0 + 1)) >= 16384) l0++;
    return scan_plan_levels(n, l0, SCAN_TOP_MAX);
}
const char* scan_plan_invalid(const ScanPlan& pl, uint64_t n) {
    if (!n) return "scan plan: no elements";
    if (n > ((uint64_t)1 << 32)) return "scan plan: more than 2^32 elements";
    if (pl.l0 < 2 || pl.l0 > 4) return "scan plan: level-0 chunk outside 2^2 .. 2^4";
    if (pl.top_max < 1 || pl.top_max > SCAN_TOP_MAX) return "scan plan: the top level takes 1 .. 2048 values";
    if (pl.K < 1) return "scan plan: no level under the top (these scans have no K = 0 form)";
    if (pl.K > SCAN_MAX_LEVELS || pl.n[pl.K] > pl.top_max) return "scan plan: more than 14 levels";
    if (pl.n[0] != n || pl.off[pl.K] + pl.n[pl.K] > scan_level_elems(n))
        return "scan plan: the stacked levels do not fit scan_level_elems(n)";
    return nullptr;
}
// what a launcher asks of a plan before it launches anything (the rest is the caller's to have checked with scan_plan_invalid;
// scan_plan's own always pass)
bool scan_plan_runs(const ScanPlan& pl, uint64_t n) {
    return n && pl.n[0] == n && pl.K >= 1 && pl.K <= SCAN_MAX_LEVELS && pl.n[pl.K] <= SCAN_TOP_MAX;
}

// The scan without its last level: chunk products of N and D up to the top, k_gp_top, the expansions back down to level 1.
// Leaves in scrN[g] / scrD[g] the exclusive prefix product of N in front of level-0 chunk g and the exclusive suffix product
// of D behind it (times 1 / prod D); returns the level-0 chunk length's log2.  N and D are only read (they may be one
// vector: the batched inversion of fr_lookup.hip).  Level 0 folds 2^l[0] elements per lane (4 for short rows, 16 for long ones,
// as the opening does), every further level 16, until at most GP_TOP_MAX values are left for k_gp_top: the plan.
int launch_gp_scan_upper(hipStream_t s, const ScanPlan& pl, const uint32_t* N, const uint32_t* D, uint64_t n, uint32_t* scrN,
                         uint32_t* scrD, uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32) {
    if (!scan_plan_runs(pl, n)) return -1;
    const int K = pl.K;
    for (int k = 0; k < K; k++)
        k_gp_chunk_prod<<<dim3(nblk(pl.n[k + 1], 256), 2), 256, 0, s>>>(k ? scrN + 8 * pl.off[k] : N, k ? scrD + 8 * pl.off[k] : D,
                                                                        pl.n[k], pl.l[k], scrN + 8 * pl.off[k + 1],
                                                                        scrD + 8 * pl.off[k + 1]);
    k_gp_top<<<1, 512, 0, s>>>(scrN + 8 * pl.off[K], scrD + 8 * pl.off[K], (uint32_t)pl.n[K], closing_be, zero_flag);
    if (start_be32) {
        FrArg st;
        memcpy(st.w, start_be32, 32);
        k_gp_chain_start<<<nblk(pl.n[K], 256), 256, 0, s>>>(scrN + 8 * pl.off[K], (uint32_t)pl.n[K], closing_be, st);
    }
    for (int k = K - 1; k >= 1; k--)
        k_gp_expand<<<dim3(nblk(pl.n[k + 1], 256), 2), 256, 0, s>>>(scrN + 8 * pl.off[k], scrD + 8 * pl.off[k], pl.n[k], pl.l[k],
                                                                    scrN + 8 * pl.off[k + 1], scrD + 8 * pl.off[k + 1]);
    return pl.l[0];
}
int launch_gp_scan_upper(hipStream_t s, const uint32_t* N, const uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                         uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32) {
    return launch_gp_scan_upper(s, scan_plan(n), N, D, n, scrN, scrD, closing_be, zero_flag, start_be32);
}
// N, D (n Montgomery elements each) -> z's evaluations in N (D is consumed).  scrN / scrD: (n + 3) / 4 * 3 / 2 + 64 elements
// of level scratch each (the sizing of the opening's h / hnext).
void launch_gp_scan(hipStream_t s, const ScanPlan& pl, uint32_t* N, uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                    uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32) {
    const int l0 = launch_gp_scan_upper(s, pl, N, D, n, scrN, scrD, closing_be, zero_flag, start_be32);
    if (l0 < 0) return;
    k_gp_final<<<nblk(pl.n[1], 256), 256, 0, s>>>(N, D, n, l0, scrN, scrD);
}
void launch_gp_scan(hipStream_t s, uint32_t* N, uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                    uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32) {
    if (n) launch_gp_scan(s, scan_plan(n), N, D, n, scrN, scrD, closing_be, zero_flag, start_be32);
}
