// fr_expr.hip -- Fr-side kernels, part 10: the expression columns of kzg_rows_commit_expr.  The quotient's term format
// (fr_quot.hip, k_quot_points) evaluated on H itself: v[t] = sum_u c_u prod_f col_{row(u,f)}[(t + rot(u,f)) mod T] for the rows
// t < n (n = usable, T in the plain layout), over source columns that lie as evaluation vectors of T elements of 8 words,
// Montgomery, CANONICAL (the forward transform ends in fr9_reduce).
//   One lane per cell t < n, 256 lanes per workgroup, one launch per expression.  The whole expression rides in ONE kernel
//   argument (1.2 KB): <= 16 coefficients as 32 big-endian bytes, <= 16 x 8 row bytes, <= 16 x 8 rotations prepared on the host
//   as rot mod T (the device does one add and one mask), the lengths.  The first lanes of every workgroup convert the
//   coefficients to Montgomery form into LDS once.  The term loop is uniform over the workgroup (trip counts and row indices
//   come from the argument), so a row pointer is a scalar load and a factor costs one 32-byte vector load and one fr9_mul.
//   Operand classes (fr29.hip.h): a coefficient in LDS is canonical; a running product is a product's output (N class, < 2r), a
//   legal FIRST operand; a loaded cell is canonical, a legal SECOND operand.  The sum is renormalised after every term: at most
//   16 terms, each below 2r (a bare coefficient below r), stay below 32r with limbs 0 .. 7 below 2^29 -- inside the 64r that
//   fr9_reduce takes, which closes with fr9_canon: a set stores canonical elements, and the zero test reads canonical words.
//   A check (STORE = false) drops the store.  Every store is a vector store.
//   Non-zero cells: counted through derive_count (ballot -> LDS -> one global add per workgroup).  The first one: the lowest
//   set bit of each wave's ballot, an LDS minimum per workgroup, one atomicMin on a u64 per workgroup -- a minimum of minima,
//   whatever the order in which the atomics return.
// Bound: 32 (factors + 1) B of traffic per cell (32 factors B for a check) against one product per factor: the multiplier
// from about two factors on.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

struct ExprArg {
    FrArg c[EXPR_MAX_TERMS];
    uint32_t rot[EXPR_MAX_TERMS][EXPR_MAX_FACTORS];
    uint8_t len[EXPR_MAX_TERMS], row[EXPR_MAX_TERMS][EXPR_MAX_FACTORS];
    uint32_t n_terms;
};
static_assert(sizeof(ExprArg) + sizeof(RowTab) + 64 <= 4096, "k_expr's arguments must fit in 4 KB");
static_assert(EXPR_MAX_FACTORS <= 255 && POLY_MAX_ROWS <= 256, "lengths and row indices ride in bytes");

// (expr_first, the workgroup's smallest flagged cell, lives in fr_kernels.hip.h beside derive_count: fr_int.hip uses it too)

// T a power of two, n <= T, every rot below T, every row below POLY_MAX_ROWS and its pointer set (the launcher's and its
// caller's checks).  Lanes t >= n read nothing and store nothing; they still walk the two reductions.
template <bool STORE>
__global__ void __launch_bounds__(256) k_expr(const RowTab rt, const ExprArg ea, uint32_t* __restrict__ out, uint64_t T, uint64_t n,
                                               unsigned long long* __restrict__ nonzero, unsigned long long* __restrict__ first) {
    __shared__ uint32_t cst[EXPR_MAX_TERMS][9];
    const uint32_t v = threadIdx.x;
    if (v < ea.n_terms) {   // (n_terms <= 16 < 256 lanes)
        uint32_t w[8];
        fr9_t c;
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = bswap32(ea.c[v].w[7 - i]);
        fr9_from_words(c, w);
        fr9_to_mont(c, c);
#pragma unroll
        for (int i = 0; i < 9; i++) cst[v][i] = c.l[i];
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + v;
    bool nz = false;
    if (t < n) {
        fr9_t acc, p, c;
        fr9_zero(acc);
        for (uint32_t u = 0; u < ea.n_terms; u++) {
#pragma unroll
            for (int i = 0; i < 9; i++) p.l[i] = cst[u][i];
            const uint32_t len = ea.len[u];
            for (uint32_t f = 0; f < len; f++) {
                fr9_load(c, rt.r[ea.row[u][f]] + 8 * ((t + ea.rot[u][f]) & (T - 1)));
                fr9_mul(p, p, c);
            }
            fr9_add(acc, acc, p);
            fr9_norm(acc, acc);
        }
        fr9_reduce(acc, acc);
        uint32_t w[8];
        fr9_to_words(w, acc);
        nz = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;
        if constexpr (STORE) {
            uint4* q = reinterpret_cast<uint4*>(out + t * 8);
            q[0] = make_uint4(w[0], w[1], w[2], w[3]);
            q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
    }
    derive_count(nz, nonzero);
    expr_first(nz, first);
}

void launch_expr(hipStream_t s, const RowTab& src, const ExprPlan& ep, uint32_t* out_or_null, uint64_t T, uint64_t n,
                 uint64_t* nonzero, uint64_t* first) {
    if (!n || n > T || (T & (T - 1)) || T > ((uint64_t)1 << 32) || ep.n_terms == 0 || ep.n_terms > EXPR_MAX_TERMS) return;
    ExprArg ea;
    memset(&ea, 0, sizeof(ea));
    ea.n_terms = ep.n_terms;
    for (uint32_t u = 0; u < ep.n_terms; u++) {
        if (ep.term_len[u] > EXPR_MAX_FACTORS) return;
        memcpy(ea.c[u].w, ep.coeffs_be32 + 32 * (size_t)u, 32);
        ea.len[u] = ep.term_len[u];
        for (uint32_t f = 0; f < ep.term_len[u]; f++) {
            if (ep.term_row[u][f] >= POLY_MAX_ROWS || !src.r[ep.term_row[u][f]] || ep.term_rot[u][f] >= T) return;
            ea.row[u][f] = ep.term_row[u][f];
            ea.rot[u][f] = ep.term_rot[u][f];
        }
    }
    auto* nzp = reinterpret_cast<unsigned long long*>(nonzero);
    auto* fp = reinterpret_cast<unsigned long long*>(first);
    if (out_or_null) k_expr<true><<<nblk(n, 256), 256, 0, s>>>(src, ea, out_or_null, T, n, nzp, fp);
    else k_expr<false><<<nblk(n, 256), 256, 0, s>>>(src, ea, nullptr, T, n, nzp, fp);
}
