// fr_poly.hip -- Fr-side kernels, part 2: the opening's evaluation y = f(alpha) and quotient (f - y) / (X - alpha) as a
// chunked linear-recurrence scan (no inversion anywhere: alpha = 0 or a root of unity need no special case), and the word
// comparison behind the row cache's verification.  Replaces eval(poly, x) and the synthetic division of worker_open
// (reference neurons/validator.py:98-104; neurons/miner.py:48).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// ------------------------------------------------------------------------------------------------ eval + quotient
// Chunk length L = 2^lchunk coefficients per lane: 16 for large polynomials, down to 4 for small rows: the chunk loops
// are chains of dependent Fr products, so short chunks + more levels beat long ones.  Inside a chain the running value
// stays lazy (product output + one canonical coefficient: < 3r) and is canonicalised once, when it is stored.
static inline int poly_lchunk(uint64_t n) {
    int l = 2;
    while (l < 4 && (n >> (l + 1)) >= 16384) l++;
    return l;
}
KZG_DEV void fr9_pow2k(fr9_t& a, int k) {  // a <- a^(2^k), canonical in and out
    for (int i = 0; i < k; i++) fr9_mul(a, a, a);
    fr9_canon(a, a);
}
// h[t] = sum_k f[t*L + k] a^k with a = alpha^(2^sq)  (sq > 0: f is itself an array of chunk values, second level)
// ARG: alpha comes as the kernel ARGUMENT (its 32 big-endian bytes) instead of from memory: the first kernel of an
// opening converts it itself -- every lane, it is one product -- and lane 0 leaves the Montgomery form at alpha_out for
// the kernels behind it (and raises *bad for a value >= r); a 1-lane conversion kernel ahead of it was ~5 us of latency
// Several rows at once (the batched opening): row blockIdx.y reads f + y * f_rs and writes h + y * h_rs (words).
// (The body is shared with the multi-point opening's pair kernels below; lead: this grid row publishes alpha.)
template <bool ARG>
KZG_DEV void poly_chunk_eval(const uint32_t* __restrict__ f, uint64_t n, int lchunk, const uint32_t* __restrict__ alpha_mont,
                             int sq, uint32_t* __restrict__ h, const FrArg& arg, bool lead, uint32_t* __restrict__ alpha_out,
                             uint32_t* __restrict__ bad) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << lchunk;
    uint64_t lo = t * L;
    fr9_t a, s, c;
    if constexpr (ARG) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = bswap32(arg.w[7 - i]);
        fr9_from_words(a, w);
        fr9_to_mont(a, a);
        if (t == 0 && lead) {
            if (fr_words_ge_r(w)) atomicOr(bad, 1u);
            fr9_store(alpha_out, a);
        }
    }
    if (lo >= n) return;
    uint64_t hi = lo + L < n ? lo + L : n;
    if constexpr (!ARG) fr9_load(a, alpha_mont);
    fr9_pow2k(a, sq);
    fr9_zero(s);
    for (uint64_t j = hi; j-- > lo;) {
        fr9_load(c, f + 8 * j);
        fr9_mul(s, s, a);
        fr9_add(s, s, c);
    }
    fr9_reduce(s, s);
    fr9_store(h + 8 * t, s);
}
template <bool ARG>
__global__ void __launch_bounds__(256) k_poly_chunk_eval(const uint32_t* __restrict__ f, uint64_t n, int lchunk,
                                                          const uint32_t* __restrict__ alpha_mont, int sq,
                                                          uint32_t* __restrict__ h, const FrArg arg,
                                                          uint32_t* __restrict__ alpha_out, uint32_t* __restrict__ bad,
                                                          uint64_t f_rs, uint64_t h_rs) {
    poly_chunk_eval<ARG>(f + blockIdx.y * f_rs, n, lchunk, alpha_mont, sq, h + blockIdx.y * h_rs, arg, blockIdx.y == 0,
                         alpha_out, bad);
}
// Suffix recurrence over chunks, H_t = h_t + beta H_{t+1}, beta = alpha^L: one NT_-lane block; lane v serially
// folds m consecutive chunks, then a Hillis-Steele suffix scan whose multiplier (beta^m)^(2^step) is uniform.
// Writes hnext[t] = H_{t+1} and y = H_0 = f(alpha).  Workgroup b scans row b: h and hnext at + b * h_rs words, y at + b.
template <uint32_t NT_>
KZG_DEV void poly_chunk_scan(uint32_t (*sm)[NT_], const uint32_t* __restrict__ h, uint64_t nchunks, int lchunk,
                             const uint32_t* __restrict__ alpha_mont, uint32_t* __restrict__ hnext,
                             uint32_t* __restrict__ y_mont, uint8_t* __restrict__ y_be_or_null) {
    const uint32_t v = threadIdx.x;
    const uint64_t m = (nchunks + NT_ - 1) / NT_;
    const uint64_t lo = (uint64_t)v * m;
    const uint64_t hi = lo + m < nchunks ? lo + m : nchunks;
    fr9_t beta, g, c, mult;
    fr9_load(beta, alpha_mont);
    fr9_pow2k(beta, lchunk);  // alpha^L
    fr9_zero(g);
    for (uint64_t u = hi; u-- > lo && lo < nchunks;) {
        fr9_load(c, h + 8 * u);
        fr9_mul(g, g, beta);
        fr9_add(g, g, c);
    }
    fr9_norm(g, g);           // < 3r, normalised
    // mult = beta^m (N class, renormalised products)
    fr9_one(mult);
    {
        fr9_t pw = beta;
        for (uint64_t e = m; e; e >>= 1) {
            if (e & 1) fr9_mul(mult, mult, pw);
            fr9_mul(pw, pw, pw);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) sm[i][v] = g.l[i];
    __syncthreads();
    for (uint32_t d = 1; d < NT_; d <<= 1) {   // g grows by < 2r per step: < 3r + 20r at the end, always normalised
        fr9_t other;
        fr9_zero(other);
        if (v + d < NT_) {
#pragma unroll
            for (int i = 0; i < 9; i++) other.l[i] = sm[i][v + d];
        }
        __syncthreads();
        fr9_mul(other, other, mult);
        fr9_add(g, g, other);
        fr9_norm(g, g);
#pragma unroll
        for (int i = 0; i < 9; i++) sm[i][v] = g.l[i];
        fr9_mul(mult, mult, mult);
        __syncthreads();
    }
    // g == H_{lo}; walk the lane's own chunks downward from H_{hi}
    fr9_t s;
    fr9_zero(s);
    if (v + 1 < NT_) {
#pragma unroll
        for (int i = 0; i < 9; i++) s.l[i] = sm[i][v + 1];
    }
    for (uint64_t u = hi; u-- > lo && lo < nchunks;) {
        fr9_t o;
        fr9_reduce(o, s);
        fr9_store(hnext + 8 * u, o);
        fr9_load(c, h + 8 * u);
        fr9_mul(s, s, beta);
        fr9_add(s, s, c);
    }
    if (v == 0) {
        fr9_reduce(s, s);
        fr9_store(y_mont, s);
        if (y_be_or_null) {   // the evaluation as the wire carries it (32 bytes big-endian): no separate 1-lane kernel
            fr9_t yc;
            fr9_from_mont(yc, s);
            uint32_t w[8];
            fr9_to_words(w, yc);
            limbs_to_be<8>(y_be_or_null, w);
        }
    }
}
template <uint32_t NT_>
__global__ void __launch_bounds__(NT_) k_poly_chunk_scan(const uint32_t* __restrict__ h, uint64_t nchunks, int lchunk,
                                                           const uint32_t* __restrict__ alpha_mont,
                                                           uint32_t* __restrict__ hnext, uint32_t* __restrict__ y_mont,
                                                           uint8_t* __restrict__ y_be_or_null, uint64_t h_rs) {
    __shared__ uint32_t sm[9][NT_];
    const uint32_t b = blockIdx.x;
    poly_chunk_scan<NT_>(sm, h + b * h_rs, nchunks, lchunk, alpha_mont, hnext + b * h_rs, y_mont + 8 * b,
                         y_be_or_null ? y_be_or_null + 32 * b : nullptr);
}
// second level back down: hnext2[g] = H_{(g+1) * L2} over groups of L2 = 2^l2 first-level chunks -> hnext[u] = H_{u+1}
KZG_DEV void poly_chunk_expand(const uint32_t* __restrict__ h, uint64_t nchunks, int l2, const uint32_t* __restrict__ alpha_mont,
                               int sq, const uint32_t* __restrict__ hnext2, uint32_t* __restrict__ hnext) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l2;
    uint64_t lo = g * L;
    if (lo >= nchunks) return;
    uint64_t hi = lo + L < nchunks ? lo + L : nchunks;
    fr9_t beta, s, c;
    fr9_load(beta, alpha_mont);
    fr9_pow2k(beta, sq);
    fr9_load(s, hnext2 + 8 * g);
    for (uint64_t u = hi; u-- > lo;) {
        fr9_t o;
        fr9_reduce(o, s);
        fr9_store(hnext + 8 * u, o);
        fr9_load(c, h + 8 * u);
        fr9_mul(s, s, beta);
        fr9_add(s, s, c);
    }
}
__global__ void __launch_bounds__(256) k_poly_chunk_expand(const uint32_t* __restrict__ h, uint64_t nchunks, int l2,
                                                            const uint32_t* __restrict__ alpha_mont, int sq,
                                                            const uint32_t* __restrict__ hnext2,
                                                            uint32_t* __restrict__ hnext) {
    poly_chunk_expand(h, nchunks, l2, alpha_mont, sq, hnext2, hnext);
}
// q[j-1] = sum_{k>=j} f_k alpha^(k-j), written canonical (ready to be MSM scalars); q has n-1 entries
// MONT: the entries stay in Montgomery form (reduced below r), the input of a further division: the chained quotients of
// kzg_rows_commit_shplonk divide by one point after the other.  Same recurrence, only the form of the stored value differs.
template <bool MONT>
KZG_DEV void poly_quotient(const uint32_t* __restrict__ f, uint64_t n, int lchunk, const uint32_t* __restrict__ alpha_mont,
                           const uint32_t* __restrict__ hnext, uint32_t* __restrict__ q_canon) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << lchunk;
    uint64_t lo = t * L;
    if (lo >= n) return;
    uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t a, s, c, o;
    fr9_load(a, alpha_mont);
    fr9_load(s, hnext + 8 * t);
    for (uint64_t j = hi; j-- > lo;) {
        fr9_load(c, f + 8 * j);
        fr9_mul(s, s, a);
        fr9_add(s, s, c);
        if (j >= 1) {
            if constexpr (MONT) fr9_reduce(o, s);
            else fr9_from_mont(o, s);
            fr9_store(q_canon + 8 * (j - 1), o);
        }
    }
    if (hi == n) {  // slot n - 1: a zero, so that the n - 1 coefficients can ride as a length-n scalar set (batched commit+open)
        fr9_zero(o);
        fr9_store(q_canon + 8 * (n - 1), o);
    }
}
__global__ void __launch_bounds__(256) k_poly_quotient(const uint32_t* __restrict__ f, uint64_t n, int lchunk,
                                                        const uint32_t* __restrict__ alpha_mont,
                                                        const uint32_t* __restrict__ hnext,
                                                        uint32_t* __restrict__ q_canon) {
    poly_quotient<false>(f, n, lchunk, alpha_mont, hnext, q_canon);
}

// ---- the multi-point opening (kzg_commit_open_multi, kzg_rows_open): grid row y is a PAIR -- row pa.row[y] at point
// pa.pt[y] -- with its own level arrays at + y * h_rs words.  The first kernel of the evaluations (ARG) reads the pair's row
// through the table rt (the row need not lie next to the others) and converts the pair's point from the kernel argument
// pa.a[pt]; the point's first pair publishes its Montgomery form at alpha_mont + 8 pt (raising *bad for a value >= r); every
// later kernel reads it from there.  The openings of the m combinations run as pairs (p, p): their level-0 input is
// f + y * f_rs.  Same bodies as the kernels above: the same arithmetic, bit for bit.
template <bool ARG>
__global__ void __launch_bounds__(256) k_poly_pairs_eval(const uint32_t* __restrict__ f, uint64_t n, int lchunk,
                                                          uint32_t* __restrict__ alpha_mont, int sq, uint32_t* __restrict__ h,
                                                          const PairArg pa, uint32_t* __restrict__ bad, uint64_t f_rs,
                                                          uint64_t h_rs, const RowTab rt) {
    const uint32_t y = blockIdx.y, p = pa.pt[y];
    poly_chunk_eval<ARG>(ARG ? rt.r[pa.row[y]] : f + y * f_rs, n, lchunk, alpha_mont + 8 * p, sq, h + y * h_rs, pa.a[p],
                         y == 0 || pa.pt[y - 1] != p, alpha_mont + 8 * p, bad);
}
template <uint32_t NT_>
__global__ void __launch_bounds__(NT_) k_poly_pairs_scan(const uint32_t* __restrict__ h, uint64_t nchunks, int lchunk,
                                                           const uint32_t* __restrict__ alpha_mont,
                                                           uint32_t* __restrict__ hnext, uint32_t* __restrict__ y_mont,
                                                           uint8_t* __restrict__ y_be_or_null, uint64_t h_rs, const PairArg pa) {
    __shared__ uint32_t sm[9][NT_];
    const uint32_t b = blockIdx.x;
    poly_chunk_scan<NT_>(sm, h + b * h_rs, nchunks, lchunk, alpha_mont + 8 * pa.pt[b], hnext + b * h_rs, y_mont + 8 * b,
                         y_be_or_null ? y_be_or_null + 32 * b : nullptr);
}
__global__ void __launch_bounds__(256) k_poly_pairs_expand(const uint32_t* __restrict__ h, uint64_t nchunks, int l2,
                                                            const uint32_t* __restrict__ alpha_mont, int sq,
                                                            const uint32_t* __restrict__ hnext2, uint32_t* __restrict__ hnext,
                                                            uint64_t h_rs, const PairArg pa) {
    const uint32_t y = blockIdx.y;
    poly_chunk_expand(h + y * h_rs, nchunks, l2, alpha_mont + 8 * pa.pt[y], sq, hnext2 + y * h_rs, hnext + y * h_rs);
}
template <bool MONT>
__global__ void __launch_bounds__(256) k_poly_pairs_quotient(const uint32_t* __restrict__ f, uint64_t n, int lchunk,
                                                              const uint32_t* __restrict__ alpha_mont,
                                                              const uint32_t* __restrict__ hnext, uint32_t* __restrict__ q_canon,
                                                              uint64_t f_rs, uint64_t h_rs, const PairArg pa) {
    const uint32_t y = blockIdx.y;
    poly_quotient<MONT>(f + y * f_rs, n, lchunk, alpha_mont + 8 * pa.pt[y], hnext + y * h_rs, q_canon + y * f_rs);
}

// ---- the batched opening's combination h[t] = sum_j gamma^j c_j[t] over k Montgomery rows at a stride of n elements
// (Horner from the last row: k - 1 dependent products per element, gamma in registers -- no table of its powers is read
// from memory).  HBM-bound: k * 32 bytes in and 32 out per element.  gamma arrives as the kernel ARGUMENT (32 big-endian
// bytes, as alpha does in k_poly_chunk_eval); every lane converts it -- one product -- and lane 0 raises *bad for a value
// >= r.  The running value stays lazy (the chunk loop's bound: <= 16 steps) and is canonicalised once, when stored.
__global__ void __launch_bounds__(256) k_fr_combine_rows(const uint32_t* __restrict__ rows, uint64_t n, uint32_t k,
                                                          const FrArg arg, uint32_t* __restrict__ out,
                                                          uint32_t* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(arg.w[7 - i]);
    if (t == 0 && fr_words_ge_r(w)) atomicOr(bad, 1u);
    if (t >= n) return;
    fr9_t g, s, c;
    fr9_from_words(g, w);
    fr9_to_mont(g, g);
    fr9_load(s, rows + 8 * ((uint64_t)(k - 1) * n + t));
    for (uint32_t j = k - 1; j-- > 0;) {
        fr9_load(c, rows + 8 * ((uint64_t)j * n + t));
        fr9_mul(s, s, g);
        fr9_add(s, s, c);
    }
    fr9_reduce(s, s);
    fr9_store(out + 8 * t, s);
}
void launch_fr_combine_rows(hipStream_t s, const uint32_t* rows_mont, uint64_t n, uint32_t k, const uint8_t gamma_be32_host[32],
                            uint32_t* out_mont, uint32_t* bad) {
    FrArg arg;
    memcpy(arg.w, gamma_be32_host, 32);
    if (n && k) k_fr_combine_rows<<<nblk(n, 256), 256, 0, s>>>(rows_mont, n, k, arg, out_mont, bad);
}

// ---- the multi-point opening's combinations: grid row p computes h_p[t] = sum_t' gamma_p^t' c_{j_t'}[t] over the rows j of
// ca.mask[p] (Horner from the highest one, as k_fr_combine_rows: one point with the full mask is its h, bit for bit) into
// out + p * n elements; row j is read at rt.r[j].  Point p's first lane raises *bad for a gamma_p >= r.
__global__ void __launch_bounds__(256) k_fr_combine_points(const RowTab rt, uint64_t n, const CombArg ca,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = blockIdx.y, mask = ca.mask[p];
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(ca.g[p].w[7 - i]);
    if (t == 0 && fr_words_ge_r(w)) atomicOr(bad, 1u);
    if (t >= n || !mask) return;
    fr9_t g, s, c;
    fr9_from_words(g, w);
    fr9_to_mont(g, g);
    int j = 31 - __clz(mask);
    fr9_load(s, rt.r[j] + 8 * t);
    while (--j >= 0) {
        if (!((mask >> j) & 1u)) continue;
        fr9_load(c, rt.r[j] + 8 * t);
        fr9_mul(s, s, g);
        fr9_add(s, s, c);
    }
    fr9_reduce(s, s);
    fr9_store(out + 8 * ((uint64_t)p * n + t), s);
}
void launch_fr_combine_points(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t m, const CombArg& ca,
                              uint32_t* out_mont, uint32_t* bad) {
    if (n && m) k_fr_combine_points<<<dim3(nblk(n, 256), m), 256, 0, s>>>(rt, n, ca, out_mont, bad);
}

// ---- the caller-weighted combinations (kzg_rows_open_lincomb): grid row p computes h_p[t] = sum_j lambda_{p,j} c_j[t] over
// the rows j of la.mask[p] (the nonzero coefficients; row j read at rt.r[j]).  HBM-bound like k_fr_combine_points: one
// product and one lazy sum per row and element.  The coefficients ride in the kernel argument as big-endian bytes; the
// first lanes of every workgroup convert the point's coefficients to Montgomery form ONCE into LDS (one product per
// coefficient, in parallel), so the element loop pays no conversion.  The sum is renormalised after every term (limbs
// < 2^30, value < 32r after 16 terms: a legal fr9_reduce input).  Workgroup (0, p) range-checks the coefficients and
// converts the point for the openings behind the launch.
struct LincArg {
    FrArg lam[POLY_MAX_POINTS][POLY_MAX_ROWS];
    FrArg a[POLY_MAX_POINTS];
    uint32_t mask[POLY_MAX_POINTS];
};
// HIP takes 4 KB of kernel arguments per launch (the CUDA limit it mirrors); this one is 2.4 KB with the table beside it
static_assert(sizeof(LincArg) + sizeof(RowTab) + 64 <= 4096, "k_fr_lincomb_points' arguments must fit in 4 KB");
__global__ void __launch_bounds__(256) k_fr_lincomb_points(const RowTab rt, uint64_t n, const LincArg la,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ alpha_mont,
                                                            uint32_t* __restrict__ bad) {
    __shared__ uint32_t lam[POLY_MAX_ROWS][9];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = blockIdx.y, mask = la.mask[p], v = threadIdx.x;
    if (v < POLY_MAX_ROWS && ((mask >> v) & 1u)) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = bswap32(la.lam[p][v].w[7 - i]);
        if (blockIdx.x == 0 && fr_words_ge_r(w)) atomicOr(bad, 1u);
        fr9_t c;
        fr9_from_words(c, w);
        fr9_to_mont(c, c);
#pragma unroll
        for (int i = 0; i < 9; i++) lam[v][i] = c.l[i];
    } else if (v == POLY_MAX_ROWS && blockIdx.x == 0 && alpha_mont) {   // the point, as the pair kernels' first level publishes it
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = bswap32(la.a[p].w[7 - i]);
        if (fr_words_ge_r(w)) atomicOr(bad, 1u);
        fr9_t a;
        fr9_from_words(a, w);
        fr9_to_mont(a, a);
        fr9_store(alpha_mont + 8 * p, a);
    }
    __syncthreads();
    if (t >= n) return;
    fr9_t s, c, l;
    fr9_zero(s);
    for (uint32_t mk = mask; mk; mk &= mk - 1) {
        const int j = __builtin_ctz(mk);
        fr9_load(c, rt.r[j] + 8 * t);
#pragma unroll
        for (int i = 0; i < 9; i++) l.l[i] = lam[j][i];
        fr9_mul(c, c, l);
        fr9_add(s, s, c);
        fr9_norm(s, s);
    }
    fr9_reduce(s, s);
    fr9_store(out + 8 * ((uint64_t)p * n + t), s);
}
void launch_fr_lincomb_points(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t m, uint32_t k, const uint8_t* coeffs_be32,
                              const uint32_t* masks, const uint8_t* points_be32, uint32_t* out_mont, uint32_t* alpha_mont,
                              uint32_t* bad) {
    if (!n || !m || m > POLY_MAX_POINTS || k > POLY_MAX_ROWS) return;
    LincArg la;
    memset(&la, 0, sizeof(la));
    for (uint32_t p = 0; p < m; p++) {
        la.mask[p] = masks[p];
        if (alpha_mont) memcpy(la.a[p].w, points_be32 + 32 * (size_t)p, 32);
        for (uint32_t j = 0; j < k; j++) memcpy(la.lam[p][j].w, coeffs_be32 + 32 * ((size_t)p * k + j), 32);
    }
    k_fr_lincomb_points<<<dim3(nblk(n, 256), m), 256, 0, s>>>(rt, n, la, out_mont, alpha_mont, bad);
}

// ---- the sum behind the chained quotients (kzg_rows_commit_shplonk): out[t] = (acc ? out[t] : 0) + sum_{g < cnt} rt.r[g][t],
// Montgomery in, reduced Montgomery out (what a row set holds).  HBM-bound: (cnt + acc) * 32 bytes in and 32 out per element.
__global__ void __launch_bounds__(256) k_fr_sum_rows(const RowTab rt, uint32_t cnt, uint64_t n, int acc, uint32_t* out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    fr9_t s, c;
    fr9_zero(s);
    if (acc) fr9_load(s, out + 8 * t);
    for (uint32_t g = 0; g < cnt; g++) {   // one sum per term, renormalised: < (cnt + 1) r <= 17 r, a legal fr9_reduce input
        fr9_load(c, rt.r[g] + 8 * t);
        fr9_add(s, s, c);
        fr9_norm(s, s);
    }
    fr9_reduce(s, s);
    fr9_store(out + 8 * t, s);
}
void launch_fr_sum_rows(hipStream_t s, const RowTab& rt, uint32_t cnt, uint64_t n, bool accumulate, uint32_t* out_mont) {
    // cnt <= POLY_MAX_ROWS is the caller's to keep (rows_shplonk_dev adds at most KZG_MAX_OPEN_POINTS vectors per launch,
    // checked there at compile time); the test only keeps a wrong caller from reading past the table
    if (n && cnt <= POLY_MAX_ROWS) k_fr_sum_rows<<<nblk(n, 256), 256, 0, s>>>(rt, cnt, n, accumulate ? 1 : 0, out_mont);
}

// ---- long rows (16 coefficients per lane): the quotient (and, as an A/B form, the level-0 fold) with the coefficients
// staged through LDS.  A lane of the kernels above walks ITS 512-byte chunk, so one wave load touches 64 pieces of 32
// bytes at a 512-byte stride (k_poly_quotient: 2.3 TB/s for 256 MB, with the caches reassembling the lines).  Here ONE
// WAVE per workgroup takes 64 consecutive chunks (32 KB of the vector) in PHASES of PQ_CO coefficients per chunk: each
// part is moved between HBM and LDS by the whole wave in 16-byte units -- a wave instruction covers whole 128-byte
// segments -- and the lanes run their recurrences out of (and, for the quotient, back into) padded LDS rows.  With four
// coefficients per phase a wave holds 9 KB of LDS and 8 staged loads: enough waves per SIMD to overlap one wave's
// transfers with another's products (uncontended: 115 us strided -> 86 us with 8 per phase -> ~70 us with 4).
// PQ_CO coefficients of every chunk per phase (8: two phases, 17-unit rows; 4: four phases, 9-unit rows -- half the LDS
// and registers per wave, twice the phases).  Row stride = 2 PQ_CO + 1 units: odd, so consecutive rows start 4 banks apart.
#ifndef PQ_CO
#define PQ_CO 4   // same-box A/B at 2^22 (profiles/r04_ab_opening_lds_phases.log): opening 0.253 (8) -> 0.236 (4) -> 0.272 ms (2)
#endif
#define PQ_ROW (2 * PQ_CO + 1)
#define PQ_PHASES (16 / PQ_CO)
#define PQ_ITERS (2 * PQ_CO)        // 16-byte units per lane and phase: 64 rows x 2 PQ_CO units / 64 lanes
KZG_DEV void pq_load_part(uint4 (*sm)[PQ_ROW], const uint4* __restrict__ src, uint32_t uoff, uint32_t lane) {
    uint4 tmp[PQ_ITERS];
#pragma unroll
    for (int i = 0; i < PQ_ITERS; i++) {   // all loads in flight before the first LDS write
        const uint32_t u = (uint32_t)i * 64 + lane;
        tmp[i] = src[(uint64_t)(u / (2 * PQ_CO)) * 32 + uoff + (u % (2 * PQ_CO))];
    }
#pragma unroll
    for (int i = 0; i < PQ_ITERS; i++) {
        const uint32_t u = (uint32_t)i * 64 + lane;
        sm[u / (2 * PQ_CO)][u % (2 * PQ_CO)] = tmp[i];
    }
}
KZG_DEV void pq_row_load(fr9_t& v, const uint4* row, int k) {
    const uint4 a = row[2 * k], b = row[2 * k + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    fr9_from_words(v, w);
}
// q[j-1] = sum_{k>=j} f_k alpha^(k-j), canonical, for the 1024 coefficients of this workgroup; q[n-1] = 0
__global__ void __launch_bounds__(64) k_poly_quotient16_lds(const uint32_t* __restrict__ f, uint64_t n,
                                                             const uint32_t* __restrict__ alpha_mont,
                                                             const uint32_t* __restrict__ hnext,
                                                             uint32_t* __restrict__ q_canon) {
    __shared__ uint4 sm[64][PQ_ROW];
    const uint32_t lane = threadIdx.x;
    const uint64_t chunk0 = (uint64_t)blockIdx.x * 64;
    const uint4* src = reinterpret_cast<const uint4*>(f) + chunk0 * 32;
    uint4* dst = reinterpret_cast<uint4*>(q_canon);
    fr9_t a, s, c, o;
    fr9_load(a, alpha_mont);
    fr9_load(s, hnext + 8 * (chunk0 + lane));
    for (int ph = 0; ph < PQ_PHASES; ph++) {
        const uint32_t uoff = (uint32_t)(PQ_PHASES - 1 - ph) * 2 * PQ_CO;
        pq_load_part(sm, src, uoff, lane);
        __syncthreads();
#pragma unroll 2
        for (int k = PQ_CO - 1; k >= 0; k--) {
            pq_row_load(c, sm[lane], k);
            fr9_mul(s, s, a);
            fr9_add(s, s, c);
            fr9_from_mont(o, s);
            uint32_t w[8];
            fr9_to_words(w, o);
            sm[lane][2 * k] = make_uint4(w[0], w[1], w[2], w[3]);       // in place: the slot the coefficient came from
            sm[lane][2 * k + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
        __syncthreads();
        // the value computed at coefficient j is q[j - 1]: the whole part moves down by one coefficient (two units)
#pragma unroll
        for (int i = 0; i < PQ_ITERS; i++) {
            const uint32_t u = (uint32_t)i * 64 + lane;
            const uint64_t gu = (chunk0 + u / (2 * PQ_CO)) * 32 + uoff + (u % (2 * PQ_CO));
            if (gu >= 2) dst[gu - 2] = sm[u / (2 * PQ_CO)][u % (2 * PQ_CO)];
        }
        __syncthreads();
    }
    if ((chunk0 + lane + 1) * 16 == n) {  // slot n - 1: a zero, so that the n - 1 coefficients ride as a length-n scalar set
        dst[2 * (n - 1)] = make_uint4(0u, 0u, 0u, 0u);
        dst[2 * (n - 1) + 1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// *flag |= 1 when the two word arrays differ anywhere (row-cache hits: the caller's row against the cached row's bytes)
__global__ void __launch_bounds__(256) k_words_differ(const uint4* __restrict__ a, const uint4* __restrict__ b, uint64_t n16,
                                                       uint32_t* __restrict__ flag) {
    uint32_t d = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 x = a[i], y = b[i];
        d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    if (__any(d != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
void launch_words_differ(hipStream_t s, const uint32_t* a, const uint32_t* b, uint64_t n_words, uint32_t* flag) {
    const uint64_t n16 = n_words / 4;   // rows are whole 32-byte elements
    if (!n16) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n16 + 255) / 256, 2048);
    k_words_differ<<<blocks, 256, 0, s>>>(reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b), n16, flag);
}

// Level 0 folds 2^l0 coefficients per lane, every further level 16 values of the level below, until at most 2048
// values are left for the single-workgroup scan; then (launch_poly_open) the suffix values H are expanded back down level
// by level.  Every serial loop is <= 16 long (each step is one dependent Fr product, ~1 us for a lone wave), and
// all levels but the scan fill the GPU.  The level arrays are stacked in h / hnext (serve.hip / pipeline.hip size them for
// (n+3)/4 * 3/2 + 64 entries; the levels above the first sum to < 1/3 of it).  `rows` rows of n coefficients (at a
// stride of n elements) go through the same launches side by side: row r's level arrays at h / hnext + r * h_row_words,
// its y at y_mont + 8 r (and y_be + 32 r) -- k evaluations for the latency of one.
// long rows: the level-0 fold and the quotient with their coefficients staged through LDS (KZG_POLY_NO_LDS=1: the
// strided forms, kept for the A/B and as the reference of test_poly_kernel_variants_agree)
static bool quotient_lds(uint64_t n, int l0) {
    static const bool no_lds = getenv("KZG_POLY_NO_LDS") != nullptr;
    // from 2^21 coefficients: same-box A/Bs (profiles/r04_ab_opening_lds_staging.log, r04_ab_opening_lds_phases.log) of the
    // opening stage: 2^22 0.284 -> 0.236 ms, 2^21 0.196 -> 0.185, 2^20 0.160 -> 0.167 (one wave per SIMD there: the LDS hop
    // is pure latency).  KZG_POLY_LDS_MIN_LOG moves the threshold.
    static const int lds_min_log = getenv("KZG_POLY_LDS_MIN_LOG") ? atoi(getenv("KZG_POLY_LDS_MIN_LOG")) : 21;
    // (the level-0 fold gains nothing from LDS staging: 53 against 49 us, profiles/r04_ab_opening_lds_staging.log -- strided)
    return !no_lds && l0 == 4 && (n & 1023) == 0 && n >= ((uint64_t)1 << lds_min_log);
}
// ---- the plan: everything the launchers below decide before they launch, as pure host arithmetic (fr_kernels.hip.h).
// Level k folds chunks of 2^l[k] of its n[k] values into the n[k + 1] values of level k + 1, whose unit is alpha^(2^sq[k + 1]);
// levels are added while the top one holds more than scan_max values (and the tables have room).
PolyPlan poly_plan_levels(uint64_t n, int l0, uint64_t scan_max, int scan_nt, bool lds) {
    PolyPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.l0 = l0;
    pl.lup = 4;   // log2 chunk of the levels above the first (4-long chunks + more levels measured no faster on short rows)
    pl.scan_max = scan_max;
    pl.scan_nt = scan_nt;
    pl.lds = lds ? 1 : 0;
    if (l0 < 2 || l0 > 4 || scan_max < 1) return pl;   // (no level table: poly_plan_invalid names the parameter)
    const int lup = pl.lup;
    int K = 1;
    pl.l[0] = l0; pl.sq[0] = 0; pl.n[0] = n; pl.off[0] = 0;           // level 0 = f itself (offset unused)
    pl.n[1] = (n + ((uint64_t)1 << l0) - 1) >> l0; pl.sq[1] = l0; pl.off[1] = 0;
    while (pl.n[K] > scan_max && K < POLY_MAX_LEVELS) {
        pl.l[K] = lup;
        pl.n[K + 1] = (pl.n[K] + ((uint64_t)1 << lup) - 1) >> lup;
        pl.sq[K + 1] = pl.sq[K] + lup;
        pl.off[K + 1] = pl.off[K] + pl.n[K];
        K++;
    }
    pl.K = K;
    return pl;
}
PolyPlan poly_plan(uint64_t n) {
    const int l0 = poly_lchunk(n);
    PolyPlan pl = poly_plan_levels(n, l0, 2048, 256, quotient_lds(n, l0));
    // the scan is one workgroup of dependent Fr products: 256 lanes (one wave per SIMD, <= 8 values each) run the chain
    // at a lone wave's issue rate; 1024 lanes (four waves per SIMD) only when there is more than that to fold
    if (pl.n[pl.K] > 1024) pl.scan_nt = 1024;
    return pl;
}
const char* poly_plan_invalid(const PolyPlan& pl, uint64_t n) {
    if (!n) return "poly plan: no coefficients";
    if (pl.l0 < 2 || pl.l0 > 4) return "poly plan: level-0 chunk outside 2^2 .. 2^4";
    if (pl.scan_max < 1) return "poly plan: the scan must be left at least one value";
    if (pl.scan_nt != 256 && pl.scan_nt != 1024) return "poly plan: the scan runs 256 or 1024 lanes";
    if (pl.K < 1 || pl.K > POLY_MAX_LEVELS || pl.n[pl.K] > pl.scan_max) return "poly plan: more than 14 levels";
    // k_poly_quotient16_lds: 16 coefficients per lane, whole workgroups of 1024 coefficients, no bounds test of its own
    if (pl.lds && (pl.l0 != 4 || (n & 1023) != 0 || n < 1024))
        return "poly plan: the LDS-staged quotient needs 16-long chunks and whole blocks of 1024 coefficients";
    if (pl.n[0] != n || (pl.off[pl.K] + pl.n[pl.K]) * 8 > poly_level_words(n))
        return "poly plan: the stacked levels do not fit poly_level_words(n)";
    return nullptr;
}
// pa given (the multi-point opening): the rows are pairs, each at its own point (k_poly_pairs_*); ARG then stands for
// alpha_be32_host != null, the points coming from pa.a and the pairs' rows from the table *rt (f_mont unused)
static void poly_up(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t rows, uint32_t* alpha_mont, uint32_t* h,
                    uint32_t* hnext, uint64_t h_rs, uint32_t* y_mont, const uint8_t* alpha_be32_host, uint32_t* bad,
                    uint8_t* y_be_or_null, const PolyPlan& lv, const PairArg* pa = nullptr, const RowTab* rt = nullptr) {
    RowTab none;
    memset(&none, 0, sizeof(none));
    const RowTab& tab = rt ? *rt : none;
    FrArg arg;
    memset(&arg, 0, sizeof(arg));
    if (alpha_be32_host) memcpy(arg.w, alpha_be32_host, 32);
    const uint64_t f_rs = rows > 1 ? n * 8 : 0;
    const int l0 = lv.l0, lup = lv.lup, K = lv.K;
    const int* lv_sq = lv.sq;
    const uint64_t* lv_n = lv.n;
    const uint64_t* lv_off = lv.off;
    if (pa) {
        if (alpha_be32_host)
            k_poly_pairs_eval<true><<<dim3(nblk(lv_n[1], 256), rows), 256, 0, s>>>(f_mont, n, l0, alpha_mont, 0, h, *pa, bad,
                                                                               n * 8, h_rs, tab);
        else
            k_poly_pairs_eval<false><<<dim3(nblk(lv_n[1], 256), rows), 256, 0, s>>>(f_mont, n, l0, alpha_mont, 0, h, *pa,
                                                                                nullptr, n * 8, h_rs, tab);
    } else if (alpha_be32_host)
        k_poly_chunk_eval<true><<<dim3(nblk(lv_n[1], 256), rows), 256, 0, s>>>(f_mont, n, l0, alpha_mont, 0, h, arg, alpha_mont,
                                                                           bad, f_rs, h_rs);
    else
        k_poly_chunk_eval<false><<<dim3(nblk(lv_n[1], 256), rows), 256, 0, s>>>(f_mont, n, l0, alpha_mont, 0, h, arg, nullptr,
                                                                            nullptr, f_rs, h_rs);
    for (int k = 1; k < K; k++) {
        if (pa)
            k_poly_pairs_eval<false><<<dim3(nblk(lv_n[k + 1], 256), rows), 256, 0, s>>>(h + 8 * lv_off[k], lv_n[k], lup,
                                                                                    alpha_mont, lv_sq[k], h + 8 * lv_off[k + 1],
                                                                                    *pa, nullptr, h_rs, h_rs, tab);
        else
            k_poly_chunk_eval<false><<<dim3(nblk(lv_n[k + 1], 256), rows), 256, 0, s>>>(h + 8 * lv_off[k], lv_n[k], lup,
                                                                                    alpha_mont, lv_sq[k], h + 8 * lv_off[k + 1],
                                                                                    arg, nullptr, nullptr, h_rs, h_rs);
    }
    if (pa) {
        if (lv.scan_nt == 256)
            k_poly_pairs_scan<256><<<rows, 256, 0, s>>>(h + 8 * lv_off[K], lv_n[K], lv_sq[K], alpha_mont, hnext + 8 * lv_off[K],
                                                        y_mont, y_be_or_null, h_rs, *pa);
        else
            k_poly_pairs_scan<1024><<<rows, 1024, 0, s>>>(h + 8 * lv_off[K], lv_n[K], lv_sq[K], alpha_mont,
                                                          hnext + 8 * lv_off[K], y_mont, y_be_or_null, h_rs, *pa);
    } else if (lv.scan_nt == 256)
        k_poly_chunk_scan<256><<<rows, 256, 0, s>>>(h + 8 * lv_off[K], lv_n[K], lv_sq[K], alpha_mont, hnext + 8 * lv_off[K],
                                                    y_mont, y_be_or_null, h_rs);
    else
        k_poly_chunk_scan<1024><<<rows, 1024, 0, s>>>(h + 8 * lv_off[K], lv_n[K], lv_sq[K], alpha_mont, hnext + 8 * lv_off[K],
                                                      y_mont, y_be_or_null, h_rs);
}
// (every launcher: the plan is the caller's to have checked with poly_plan_invalid; poly_plan's own always pass)
void launch_poly_open(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t* alpha_mont, uint32_t* h,
                      uint32_t* hnext, uint32_t* y_mont, uint32_t* q_canon_or_null, const uint8_t* alpha_be32_host,
                      uint32_t* bad, uint8_t* y_be_or_null) {
    launch_poly_open(s, poly_plan(n), f_mont, n, alpha_mont, h, hnext, y_mont, q_canon_or_null, alpha_be32_host, bad,
                     y_be_or_null);
}
void launch_poly_open(hipStream_t s, const PolyPlan& lv, const uint32_t* f_mont, uint64_t n, uint32_t* alpha_mont, uint32_t* h,
                      uint32_t* hnext, uint32_t* y_mont, uint32_t* q_canon_or_null, const uint8_t* alpha_be32_host,
                      uint32_t* bad, uint8_t* y_be_or_null) {
    if (!n) {
        if (alpha_be32_host) launch_fr_from_host32(s, alpha_be32_host, alpha_mont, 1, bad);
        return;
    }
    poly_up(s, f_mont, n, 1, alpha_mont, h, hnext, 0, y_mont, alpha_be32_host, bad, y_be_or_null, lv);
    const int l0 = lv.l[0], K = lv.K;
    const int* lv_l = lv.l;
    const int* lv_sq = lv.sq;
    const uint64_t* lv_n = lv.n;
    const uint64_t* lv_off = lv.off;
    const bool lds = lv.lds != 0;
    for (int k = K - 1; k >= 1; k--)
        k_poly_chunk_expand<<<nblk(lv_n[k + 1], 256), 256, 0, s>>>(h + 8 * lv_off[k], lv_n[k], lv_l[k], alpha_mont,
                                                                   lv_sq[k], hnext + 8 * lv_off[k + 1],
                                                                   hnext + 8 * lv_off[k]);
    if (q_canon_or_null) {
        if (lds) k_poly_quotient16_lds<<<(uint32_t)(n >> 10), 64, 0, s>>>(f_mont, n, alpha_mont, hnext, q_canon_or_null);
        else k_poly_quotient<<<nblk(lv_n[1], 256), 256, 0, s>>>(f_mont, n, l0, alpha_mont, hnext, q_canon_or_null);
    }
}
void launch_poly_eval_rows(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t rows, uint32_t* alpha_mont,
                           uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                           const uint8_t* alpha_be32_host, uint32_t* bad, uint8_t* y_be) {
    if (n && rows)
        launch_poly_eval_rows(s, poly_plan(n), f_mont, n, rows, alpha_mont, h, hnext, h_row_words, y_mont, alpha_be32_host, bad,
                              y_be);
}
void launch_poly_eval_rows(hipStream_t s, const PolyPlan& lv, const uint32_t* f_mont, uint64_t n, uint32_t rows,
                           uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                           const uint8_t* alpha_be32_host, uint32_t* bad, uint8_t* y_be) {
    if (n && rows) poly_up(s, f_mont, n, rows, alpha_mont, h, hnext, h_row_words, y_mont, alpha_be32_host, bad, y_be, lv);
}

void launch_poly_eval_pairs(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t npairs, const PairArg& pa,
                            uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                            uint32_t* bad, uint8_t* y_be) {
    if (n && npairs)
        launch_poly_eval_pairs(s, poly_plan(n), rt, n, npairs, pa, alpha_mont, h, hnext, h_row_words, y_mont, bad, y_be);
}
void launch_poly_eval_pairs(hipStream_t s, const PolyPlan& lv, const RowTab& rt, uint64_t n, uint32_t npairs, const PairArg& pa,
                            uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                            uint32_t* bad, uint8_t* y_be) {
    static const uint8_t ARG_MARK[32] = {};   // (non-null: the first kernel converts the points of pa.a)
    if (n && npairs)
        poly_up(s, nullptr, n, npairs, alpha_mont, h, hnext, h_row_words, y_mont, ARG_MARK, bad, y_be, lv, &pa, &rt);
}
// the levels go up with the pair kernels (pair p = combination p at point p), then back down as in launch_poly_open with
// grid y = point; long rows' LDS-staged quotient runs once per point
// pts (the chained divisions of kzg_rows_commit_shplonk): vector p is divided by the point alpha_mont + 8 pts[p] instead of
// point p, and q_mont keeps the quotients in Montgomery form for the next division (always the strided quotient kernel)
void launch_poly_open_points(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t m, const uint32_t* alpha_mont,
                             uint32_t* h, uint32_t* hnext, uint64_t h_rs, uint32_t* y_mont, uint32_t* q_canon,
                             uint8_t* y_be, const uint8_t* pts, bool q_mont) {
    if (!n || !m || m > POLY_MAX_POINTS) return;
    launch_poly_open_points(s, poly_plan(n), f_mont, n, m, alpha_mont, h, hnext, h_rs, y_mont, q_canon, y_be, pts, q_mont);
}
void launch_poly_open_points(hipStream_t s, const PolyPlan& lv, const uint32_t* f_mont, uint64_t n, uint32_t m,
                             const uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_rs, uint32_t* y_mont,
                             uint32_t* q_canon, uint8_t* y_be, const uint8_t* pts, bool q_mont) {
    // m <= POLY_MAX_POINTS is the caller's to keep (the C-ABI refuses more points; rows_shplonk_dev batches its groups by
    // KZG_MAX_OPEN_POINTS, checked at compile time); the test only keeps a wrong caller from writing past PairArg
    if (!n || !m || m > POLY_MAX_POINTS) return;
    PairArg pa;
    memset(&pa, 0, sizeof(pa));
    for (uint32_t p = 0; p < m; p++) {
        pa.row[p] = (uint8_t)p;
        pa.pt[p] = pts ? pts[p] : (uint8_t)p;
    }
    uint32_t* am = const_cast<uint32_t*>(alpha_mont);   // (read only: no point is converted on this path)
    poly_up(s, f_mont, n, m, am, h, hnext, h_rs, y_mont, nullptr, nullptr, y_be, lv, &pa);
    const int l0 = lv.l[0], K = lv.K;
    for (int k = K - 1; k >= 1; k--)
        k_poly_pairs_expand<<<dim3(nblk(lv.n[k + 1], 256), m), 256, 0, s>>>(h + 8 * lv.off[k], lv.n[k], lv.l[k], alpha_mont,
                                                                            lv.sq[k], hnext + 8 * lv.off[k + 1],
                                                                            hnext + 8 * lv.off[k], h_rs, pa);
    if (q_mont) {
        k_poly_pairs_quotient<true><<<dim3(nblk(lv.n[1], 256), m), 256, 0, s>>>(f_mont, n, l0, alpha_mont, hnext, q_canon, n * 8,
                                                                                h_rs, pa);
    } else if (lv.lds) {
        for (uint32_t p = 0; p < m; p++)
            k_poly_quotient16_lds<<<(uint32_t)(n >> 10), 64, 0, s>>>(f_mont + p * n * 8, n, alpha_mont + 8 * pa.pt[p],
                                                                    hnext + p * h_rs, q_canon + p * n * 8);
    } else {
        k_poly_pairs_quotient<false><<<dim3(nblk(lv.n[1], 256), m), 256, 0, s>>>(f_mont, n, l0, alpha_mont, hnext, q_canon, n * 8,
                                                                          h_rs, pa);
    }
}
