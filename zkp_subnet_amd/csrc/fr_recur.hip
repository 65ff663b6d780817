// fr_recur.hip -- Fr-side kernels, part 11: the first-order recurrence columns of kzg_rows_commit_recurrence.
//   v[0] = start, v[t + 1] = A[t] v[t] + B[t] for t < n, over two vectors A, B of canonical Montgomery elements (8 words each)
// is the inclusive scan of the affine maps x -> A[t] x + B[t] under composition,
//   (A2, B2) o (A1, B1) = (A2 A1, A2 B1 + B2)      ((A1, B1) applied first),
// run as the ladder of the product scan (fr_prod.hip), the sum scan (fr_lookup.hip) and the opening's Horner scan (fr_poly.hip),
// with a pair as the element and two products and one sum as the operator.
//   way up      k_recur_fold   level k folds chunks of 2^l[k] maps into one map of level k + 1, one lane per chunk (level 0: the
//               vectors A, B themselves; 2^l0 per lane, 16 above) until at most top_max <= RECUR_TOP_MAX maps are left
//   top         k_recur_top    ONE workgroup of 256 lanes: a lane folds its <= 8 maps, a Hillis-Steele scan over the 256 lane
//               maps in LDS (2 x 9 x 256 words, 18 KB, limb-major: lane v reads word v of every row, no bank conflict) gives
//               each lane the map in front of it, which it applies to `start`: FROM HERE DOWN THE LADDER CARRIES VALUES, NOT
//               MAPS.  Each top map's A slot takes the value in front of it; the total applied to start is the closing value
//   way down    k_recur_walk   the lane of a chunk starts from the value in its parent's A slot and walks val <- A val + B, one
//               product per element, storing the value IN FRONT of every element over that element's A slot; the level-0 walk
//               stores into the output vector: out[t] = v[t]
// The A and B parts of every level lie in two scratch arrays at the same element offsets (level 0: the callers' vectors), so all
// three kernels read "element u of A, element u of B" whatever the level.
// Operand classes (fr29.hip.h): every element that is loaded is canonical -- a legal operand on either side of fr9_mul.  A
// product is N class (< 2r, limbs 0 .. 7 below 2^29); A2 A1 is made canonical by fr9_canon; A2 B1 + B2 is a product plus a
// canonical value (< 3r, limbs below 2^30), normalised and made canonical by fr9_reduce.  Every register value that enters a
// further product or a store is therefore canonical; everything the set stores is canonical.  Empty lanes of a partial top
// level carry the identity (1, 0).  A zero multiplier is no special case: (0, B) o anything = (0, B), the segment restart.
// Every store is a vector store (fr9_store: two 16-byte stores) or plain C++.
// Cost: per level-0 element (2^l0 - 1) / 2^l0 compositions of two products on the way up and one product on the way down,
// about three products per cell; traffic 2 x 32 B read on the way up, 2 x 32 B read and 32 B written on the way down, plus the
// upper levels' 1 / 2^l0 share: about 220 B per cell.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// (a, b) <- (a2, b2) o (a, b): the map (a, b) first, (a2, b2) behind it.  All four canonical in, canonical out
KZG_DEV void recur_compose(fr9_t& a, fr9_t& b, const fr9_t& a2, const fr9_t& b2) {
    fr9_t t;
    fr9_mul(t, a2, a);
    fr9_canon(a, t);
    fr9_mul(t, a2, b);
    fr9_add(t, t, b2);
    fr9_reduce(b, t);
}
// val <- a val + b, canonical in and out
KZG_DEV void recur_apply(fr9_t& val, const fr9_t& a, const fr9_t& b) {
    fr9_t t;
    fr9_mul(t, a, val);
    fr9_add(t, t, b);
    fr9_reduce(val, t);
}

// one level up: map g of the output is the composition of the maps [g 2^l, min((g + 1) 2^l, n)) of the input, in their order.
// The output arrays hold ceil(n / 2^l) elements (the launcher's plan); a lane whose chunk starts at or behind n does nothing
__global__ void __launch_bounds__(256) k_recur_fold(const uint32_t* __restrict__ Ain, const uint32_t* __restrict__ Bin, uint64_t n,
                                                     int l, uint32_t* __restrict__ Aout, uint32_t* __restrict__ Bout) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t a, b, a2, b2;
    fr9_load(a, Ain + 8 * lo);
    fr9_load(b, Bin + 8 * lo);
    for (uint64_t u = lo + 1; u < hi; u++) {
        fr9_load(a2, Ain + 8 * u);
        fr9_load(b2, Bin + 8 * u);
        recur_compose(a, b, a2, b2);
    }
    fr9_store(Aout + 8 * g, a);
    fr9_store(Bout + 8 * g, b);
}

// The top level, one workgroup of 256 lanes over m >= 1 maps (the plan keeps m <= RECUR_TOP_MAX: <= 8 per lane; any m is
// computed correctly).  vout[u] <- the value in front of map u (vout may be A itself: a lane loads its element before it stores
// over it, and no lane touches another lane's elements); closing_be <- the value behind the last map, 32 big-endian bytes;
// close_row (null: none) <- the same value as a canonical Montgomery element
__global__ void __launch_bounds__(256) k_recur_top(const uint32_t* A, const uint32_t* __restrict__ B, uint32_t m, const FrArg start,
                                                    uint32_t* vout, uint8_t* __restrict__ closing_be, uint32_t* __restrict__ close_row) {
    __shared__ uint32_t sa[9][256], sb[9][256];
    const uint32_t v = threadIdx.x;
    const uint32_t per = (m + 255u) / 256u;
    const uint32_t lo = v * per < m ? v * per : m, hi = lo + per < m ? lo + per : m;
    fr9_t a, b, a2, b2;
    fr9_one(a);      // the identity (1, 0): Montgomery 1
    fr9_zero(b);
    for (uint32_t u = lo; u < hi; u++) {
        fr9_load(a2, A + 8 * (uint64_t)u);
        fr9_load(b2, B + 8 * (uint64_t)u);
        recur_compose(a, b, a2, b2);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        sa[i][v] = a.l[i];
        sb[i][v] = b.l[i];
    }
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        fr9_t oa, ob;
        const bool has = v >= d;
        if (has) {
#pragma unroll
            for (int i = 0; i < 9; i++) {
                oa.l[i] = sa[i][v - d];
                ob.l[i] = sb[i][v - d];
            }
        }
        __syncthreads();
        if (has) {
            recur_compose(oa, ob, a, b);   // the lanes in front first, this lane's map behind them
            a = oa;
            b = ob;
#pragma unroll
            for (int i = 0; i < 9; i++) {
                sa[i][v] = a.l[i];
                sb[i][v] = b.l[i];
            }
        }
        __syncthreads();
    }
    // (sa, sb)[.][v] = the composition of the maps of lanes 0 .. v; lane 255's is the whole level
    fr9_t st, val;
    {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = bswap32(start.w[7 - i]);
        fr9_from_words(st, w);
        fr9_to_mont(st, st);
    }
    if (v == 255) {
        val = st;
        recur_apply(val, a, b);
        if (close_row) fr9_store(close_row, val);
        fr9_t cl;
        fr9_from_mont(cl, val);
        uint32_t w[8];
        fr9_to_words(w, cl);
        limbs_to_be<8>(closing_be, w);
    }
    val = st;
    if (v) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            a.l[i] = sa[i][v - 1];
            b.l[i] = sb[i][v - 1];
        }
        recur_apply(val, a, b);
    }
    for (uint32_t u = lo; u < hi; u++) {
        fr9_load(a2, A + 8 * (uint64_t)u);
        fr9_load(b2, B + 8 * (uint64_t)u);
        fr9_store(vout + 8 * (uint64_t)u, val);
        if (u + 1 < hi) recur_apply(val, a2, b2);
    }
}

// one level down: chunk g of 2^l elements of this level starts from the value vin[g] in front of it (its parent's A slot);
// vout[u] <- the value in front of element u (vout may be A itself, as in k_recur_top).  At level 0 that is v[u]
__global__ void __launch_bounds__(256) k_recur_walk(const uint32_t* A, const uint32_t* __restrict__ B, uint64_t n, int l,
                                                     const uint32_t* __restrict__ vin, uint32_t* vout) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t L = (uint64_t)1 << l, lo = g * L;
    if (lo >= n) return;
    const uint64_t hi = lo + L < n ? lo + L : n;
    fr9_t val, a, b;
    fr9_load(val, vin + 8 * g);
    for (uint64_t u = lo; u < hi; u++) {
        fr9_load(a, A + 8 * u);
        fr9_load(b, B + 8 * u);
        fr9_store(vout + 8 * u, val);
        if (u + 1 < hi) recur_apply(val, a, b);
    }
}

// ---- the plan: pure host arithmetic (fr_kernels.hip.h).  Level k holds n[k] maps; level 0 is the vectors themselves, level
// k >= 1 starts at element off[k] of both scratch arrays; levels are added while the top one holds more than top_max maps
// (the product and the additive scan share the loop with min_levels = 1: they always fold level 0 once, scan_plan_levels)
RecurPlan ladder_plan_levels(uint64_t n, int l0, uint64_t top_max, int min_levels) {
    RecurPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.l0 = l0;
    pl.lup = 4;
    pl.top_max = top_max;
    pl.n[0] = n;
    if (l0 < 2 || l0 > 4 || top_max < 1) return pl;   // (no level table: recur_plan_invalid names the parameter)
    int K = 0;
    while ((pl.n[K] > top_max || K < min_levels) && K < RECUR_MAX_LEVELS) {
        pl.l[K] = K ? pl.lup : l0;
        pl.n[K + 1] = (pl.n[K] + ((uint64_t)1 << pl.l[K]) - 1) >> pl.l[K];
        pl.off[K + 1] = K ? pl.off[K] + pl.n[K] : 0;
        K++;
    }
    pl.K = K;
    return pl;
}
RecurPlan recur_plan_levels(uint64_t n, int l0, uint64_t top_max) { return ladder_plan_levels(n, l0, top_max, 0); }
RecurPlan recur_plan(uint64_t n) {
    const int l0 = n < ((uint64_t)1 << 17) ? 2 : n < ((uint64_t)1 << 18) ? 3 : 4;
    return recur_plan_levels(n, l0, RECUR_TOP_MAX);
}
const char* recur_plan_invalid(const RecurPlan& pl, uint64_t n) {
    if (!n) return "recur plan: no rows";
    if (n > ((uint64_t)1 << 32)) return "recur plan: more than 2^32 rows";
    if (pl.l0 < 2 || pl.l0 > 4) return "recur plan: level-0 chunk outside 2^2 .. 2^4";
    if (pl.top_max < 1 || pl.top_max > RECUR_TOP_MAX) return "recur plan: the top level takes 1 .. 2048 maps";
    if (pl.K < 0 || pl.K > RECUR_MAX_LEVELS || pl.n[pl.K] > pl.top_max) return "recur plan: more than 14 levels";
    if (pl.n[0] != n || (pl.K && pl.off[pl.K] + pl.n[pl.K] > recur_level_elems(n)))
        return "recur plan: the stacked levels do not fit recur_level_elems(n)";
    return nullptr;
}

// (the plan is the caller's to have checked with recur_plan_invalid; recur_plan's own always pass)
void launch_recur_scan(hipStream_t s, const RecurPlan& pl, const uint32_t* A, const uint32_t* B, uint64_t n, uint32_t* scrA,
                       uint32_t* scrB, const uint8_t start_be32[32], uint32_t* out, uint8_t* closing_be, uint32_t* close_row) {
    if (!n || pl.n[0] != n || pl.K < 0 || pl.K > RECUR_MAX_LEVELS || pl.n[pl.K] > RECUR_TOP_MAX) return;
    const int K = pl.K;
    FrArg st;
    memcpy(st.w, start_be32, 32);
    auto a_of = [&](int k) { return k ? scrA + 8 * pl.off[k] : A; };
    auto b_of = [&](int k) { return k ? scrB + 8 * pl.off[k] : B; };
    for (int k = 0; k < K; k++)
        k_recur_fold<<<nblk(pl.n[k + 1], 256), 256, 0, s>>>(a_of(k), b_of(k), pl.n[k], pl.l[k], scrA + 8 * pl.off[k + 1],
                                                           scrB + 8 * pl.off[k + 1]);
    k_recur_top<<<1, 256, 0, s>>>(a_of(K), b_of(K), (uint32_t)pl.n[K], st, K ? scrA + 8 * pl.off[K] : out, closing_be, close_row);
    for (int k = K - 1; k >= 0; k--)
        k_recur_walk<<<nblk(pl.n[k + 1], 256), 256, 0, s>>>(a_of(k), b_of(k), pl.n[k], pl.l[k], scrA + 8 * pl.off[k + 1],
                                                           k ? scrA + 8 * pl.off[k] : out);
}
void launch_recur_scan(hipStream_t s, const uint32_t* A, const uint32_t* B, uint64_t n, uint32_t* scrA, uint32_t* scrB,
                       const uint8_t start_be32[32], uint32_t* out, uint8_t* closing_be, uint32_t* close_row) {
    if (n) launch_recur_scan(s, recur_plan(n), A, B, n, scrA, scrB, start_be32, out, closing_be, close_row);
}
