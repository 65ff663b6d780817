// fr_sort.hip -- Fr-side kernels, part 8: the stable sort of kzg_rows_commit_sorted.  The w columns of the call lie as evaluation
// vectors (T elements of 8 words, Montgomery, canonical: the forward transform ends in fr9_reduce); rows [0, n) are ordered
// by the CANONICAL INTEGERS of the first n_keys columns, column 0 most significant, ties by ascending source row.  Montgomery
// words do not order like the values, so the keys leave Montgomery form once, into a key buffer of n_keys vectors.
//
// An LSD radix sort over a u32 permutation, 8-bit digits: pass p reads byte p % 32 of key column n_keys - 1 - p / 32, so the
// last pass is the top byte of column 0.  32 n_keys passes at most, and only those that move anything:
//   keys    : one lane per (row, key column): the key's canonical words into the key buffer, and the digit histograms of the
//             column's 32 passes in ONE sweep (LDS, then one global add per workgroup and non-empty bin)
//   plan    : per pass, skip[p] = "one bin holds all n rows" (the pass is the identity on a stable sort) and the histogram
//             becomes the exclusive bases of the bins.  The host reads the <= 512 skip words back: the ONE synchronisation
//             of the sort, after which only the passes that move something are launched (a column of 16-bit values costs two)
//   count   : per tile of SORT_TILE positions of the current order: the digit of every position (kept in a byte vector for
//             the scatter) and the tile's 256 counts
//   offsets : per digit, the exclusive scan of its counts over the tiles, on top of the bin's base
//   scatter : the tile again: every position's rank among the equal digits of its tile, by POSITION (below), and the store
//             of its row index to bin offset + rank
//   gather  : out[t] = column[perm[t]], one launch per column;  tail: the usable layout's rows [usable, T) from the caller
// Stable and deterministic: a wave owns a contiguous run of the tile and walks it in rounds of 64 positions; in a round the
// lanes with one digit find each other with eight ballots (sort_match8), a lane's rank is the count of LOWER lanes of its
// group plus what the wave has counted for the digit in earlier rounds (a per-wave LDS counter that only the group's lowest
// lane writes: no atomic), and the waves' totals are chained in wave order.  No rank ever depends on the order in which an
// atomic returns; the only atomics are the histogram adds of `keys`, whose sums do not depend on their order.  A constant
// digit does not serialise anything: a group of 64 equal lanes is one LDS add (keys) or one LDS store (count, scatter).
// Bounds: keys is one Montgomery product per element and key column; every other kernel moves bytes -- count chases one
// dependent 4-byte load per position (perm -> key word), scatter stores 4 bytes per position to a data-dependent address.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

#define SORT_WAVES 4
#define SORT_ROUNDS 8
#define SORT_TILE (SORT_WAVES * SORT_ROUNDS * 64)   // 2048 positions per workgroup of count / scatter
#define SORT_KEY_BLOCKS 256                         // workgroups per key column of `keys` (grid-stride over the rows)

// the lanes of `active` whose 8-bit digit equals this lane's.  Called by the whole wave (uniform control flow).
KZG_DEV uint64_t sort_match8(uint32_t d, uint64_t active) {
    uint64_t m = active;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}
KZG_DEV uint64_t sort_lanes_below() { return ((uint64_t)1 << (threadIdx.x & 63u)) - 1; }

// ------------------------------------------------------------------------------------------------ keys + histograms
// grid (<= SORT_KEY_BLOCKS, n_keys).  Operand classes (fr29.hip.h): the loaded element is canonical (limbs < 2^29, value < r),
// a legal FIRST operand of fr9_mul; the second operand is the integer 1 (normalised); the product a * 1 / R is class N (< 2r);
// fr9_canon brings it into [0, r): the element's canonical integer, whose 8 words are the key.
__global__ void __launch_bounds__(256) k_sort_keys(const uint32_t* __restrict__ ev, uint32_t* __restrict__ keys, uint64_t T,
                                                    uint32_t n, uint32_t n_keys, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[32 * 256];
    for (uint32_t j = threadIdx.x; j < 32 * 256; j += 256) h[j] = 0;
    __syncthreads();
    const uint32_t c = blockIdx.y;
    const uint64_t below = sort_lanes_below();
    for (uint64_t t0 = (uint64_t)blockIdx.x * 256; t0 < n; t0 += (uint64_t)gridDim.x * 256) {
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < n;
        uint32_t w[8] = {};
        if (live) {
            fr9_t v;
            fr9_load(v, ev + ((uint64_t)c * T + t) * 8);
            fr9_from_mont(v, v);
            fr9_to_words(w, v);
            uint4* q = reinterpret_cast<uint4*>(keys + ((uint64_t)c * T + t) * 8);
            q[0] = make_uint4(w[0], w[1], w[2], w[3]);
            q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
        const uint64_t active = __ballot(live);
#pragma unroll
        for (int b = 0; b < 32; b++) {
            const uint32_t d = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
            const uint64_t m = sort_match8(d, active);
            if (live && (m & below) == 0) atomicAdd(&h[b * 256 + d], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    uint32_t* g = hist + (uint64_t)(n_keys - 1 - c) * 32 * 256;   // the column's passes: byte b is pass 32 (n_keys - 1 - c) + b
    for (uint32_t j = threadIdx.x; j < 32 * 256; j += 256)
        if (h[j]) atomicAdd(g + j, h[j]);
}

// block-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix, *total the sum
KZG_DEV uint32_t sort_block_scan(uint32_t v, uint32_t* sh /* 256 */, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}
// grid = passes: hist[p][.] counts -> exclusive bases; skip[p] = some bin holds all n rows
__global__ void __launch_bounds__(256) k_sort_plan(uint32_t* __restrict__ hist, uint32_t n, uint32_t* __restrict__ skip) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t full;
    if (threadIdx.x == 0) full = 0;
    __syncthreads();
    uint32_t* hp = hist + (uint64_t)blockIdx.x * 256;
    const uint32_t cnt = hp[threadIdx.x];
    if (cnt == n) full = 1;
    uint32_t total;
    hp[threadIdx.x] = sort_block_scan(cnt, sh, &total);
    if (threadIdx.x == 0) skip[blockIdx.x] = full;
}

// ------------------------------------------------------------------------------------------------ one pass
// The walk count and scatter share.  Wave wv of tile `tile` owns positions [tile * SORT_TILE + wv * SORT_ROUNDS * 64, + SORT_ROUNDS
// * 64), round r its positions + r * 64 + lane.
// count: grid = tiles.  perm_in null: the identity (the first pass that runs).  cnt_out[d * ntiles + tile] <- the tile's count of d
__global__ void __launch_bounds__(256) k_sort_count(const uint32_t* __restrict__ keys, uint64_t word0, uint32_t shift,
                                                     const uint32_t* __restrict__ perm_in, uint32_t n,
                                                     uint8_t* __restrict__ digit, uint32_t* __restrict__ cnt_out, uint32_t ntiles) {
    __shared__ uint32_t cnt[SORT_WAVES][256];
    for (uint32_t j = threadIdx.x; j < SORT_WAVES * 256; j += 256) (&cnt[0][0])[j] = 0;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t below = sort_lanes_below();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wv * SORT_ROUNDS * 64;
    for (int r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t pos = base + (uint64_t)r * 64 + lane;
        const bool live = pos < n;
        uint32_t d = 0;
        if (live) {
            const uint32_t src = perm_in ? perm_in[pos] : (uint32_t)pos;
            d = (keys[word0 + (uint64_t)src * 8] >> shift) & 0xffu;
            digit[pos] = (uint8_t)d;
        }
        const uint64_t m = sort_match8(d, __ballot(live));
        if (live && (m & below) == 0) cnt[wv][d] += (uint32_t)__popcll(m);   // one lane per digit of the round: no atomic
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    const uint32_t dg = threadIdx.x;
    cnt_out[(uint64_t)dg * ntiles + blockIdx.x] = cnt[0][dg] + cnt[1][dg] + cnt[2][dg] + cnt[3][dg];
}
// offsets: grid = 256 digits.  cnt[d][0 .. ntiles) <- base[d] + its exclusive scan, in place
__global__ void __launch_bounds__(256) k_sort_offsets(uint32_t* __restrict__ cnt, uint32_t ntiles, const uint32_t* __restrict__ base) {
    __shared__ uint32_t sh[256];
    uint32_t* row = cnt + (uint64_t)blockIdx.x * ntiles;
    const uint32_t per = (ntiles + 255) / 256;
    const uint64_t lo = (uint64_t)threadIdx.x * per;
    const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
    uint32_t sum = 0;
    for (uint64_t j = lo; j < hi; j++) sum += row[j];
    uint32_t total;
    uint32_t run = base[blockIdx.x] + sort_block_scan(sum, sh, &total);
    for (uint64_t j = lo; j < hi; j++) {
        const uint32_t c = row[j];
        row[j] = run;
        run += c;
    }
}
// scatter: grid = tiles.  perm_out[off[d][tile] + rank in the tile among the positions with digit d] <- the position's row
__global__ void __launch_bounds__(256) k_sort_scatter(const uint8_t* __restrict__ digit, const uint32_t* __restrict__ perm_in,
                                                       uint32_t* __restrict__ perm_out, uint32_t n,
                                                       const uint32_t* __restrict__ off, uint32_t ntiles) {
    __shared__ uint32_t cnt[SORT_WAVES][256];
    for (uint32_t j = threadIdx.x; j < SORT_WAVES * 256; j += 256) (&cnt[0][0])[j] = 0;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t below = sort_lanes_below();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wv * SORT_ROUNDS * 64;
    uint32_t src[SORT_ROUNDS], dd[SORT_ROUNDS], loc[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t pos = base + (uint64_t)r * 64 + lane;
        const bool live = pos < n;
        dd[r] = live ? digit[pos] : 0u;
        src[r] = live ? (perm_in ? perm_in[pos] : (uint32_t)pos) : 0u;
        const uint64_t m = sort_match8(dd[r], __ballot(live));
        const uint32_t before = live ? cnt[wv][dd[r]] : 0u;   // what the wave's earlier rounds counted for this digit
        __builtin_amdgcn_wave_barrier();
        loc[r] = before + (uint32_t)__popcll(m & below);
        if (live && (m & below) == 0) cnt[wv][dd[r]] = before + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // the waves' totals chained in wave order behind the tile's offset: cnt[wv][d] becomes the wave's first slot of d
        const uint32_t dg = threadIdx.x;
        uint32_t o = off[(uint64_t)dg * ntiles + blockIdx.x];
#pragma unroll
        for (int v = 0; v < SORT_WAVES; v++) {
            const uint32_t c = cnt[v][dg];
            cnt[v][dg] = o;
            o += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++) {
        const uint64_t pos = base + (uint64_t)r * 64 + lane;
        if (pos < n) {
            const uint32_t dst = cnt[wv][dd[r]] + loc[r];
            if (dst < n) perm_out[dst] = src[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------ gather + tail
// out[t] = col[perm[t]] for t < n (perm null: the identity); rows [n, T) of out are the tail kernel's
__global__ void __launch_bounds__(256) k_sort_gather(const uint32_t* __restrict__ col, const uint32_t* __restrict__ perm,
                                                      uint32_t* __restrict__ out, uint32_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t s = perm ? perm[t] : t;
    const uint4* q = reinterpret_cast<const uint4*>(col + s * 8);
    const uint4 a = q[0], b = q[1];
    uint4* o = reinterpret_cast<uint4*>(out + t * 8);
    o[0] = a;
    o[1] = b;
}
// v[usable + j] <- tail[j] in Montgomery form for j < cnt <= BLIND_MAX_ROWS: one column's tail rides in the kernel argument
struct SortTail {
    FrArg v[BLIND_MAX_ROWS];
};
__global__ void __launch_bounds__(64) k_sort_tail(uint32_t* __restrict__ v, uint64_t usable, uint32_t cnt, const SortTail tail,
                                                   uint32_t* __restrict__ bad) {
    const uint32_t j = threadIdx.x;
    if (j >= BLIND_MAX_ROWS || j >= cnt) return;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(tail.v[j].w[7 - i]);
    if (fr_words_ge_r(w)) atomicOr(bad, 1u);
    fr9_t x;
    fr9_from_words(x, w);
    fr9_to_mont(x, x);
    fr9_store(v + 8 * (usable + j), x);
}

// ------------------------------------------------------------------------------------------------ launchers
// the workspace behind the key buffer, in words: two permutations, the digit bytes, the per-tile counts, the histograms of all
// passes and the skip words
struct SortWs {
    uint32_t *perm[2], *tile_cnt, *hist, *skip;
    uint8_t* digit;
    uint32_t ntiles, passes;
    uint64_t words;
};
static SortWs sort_ws(uint32_t* ws, uint64_t n, uint32_t n_keys) {
    auto up4 = [](uint64_t x) { return (x + 3) & ~(uint64_t)3; };   // 16-byte pieces
    SortWs s;
    s.ntiles = nblk(n, SORT_TILE);
    s.passes = 32 * n_keys;
    uint64_t o = 0;
    s.perm[0] = ws + o; o += up4(n);
    s.perm[1] = ws + o; o += up4(n);
    s.digit = reinterpret_cast<uint8_t*>(ws + o); o += up4((n + 3) / 4);
    s.tile_cnt = ws + o; o += up4((uint64_t)256 * s.ntiles);
    s.hist = ws + o; o += (uint64_t)s.passes * 256;
    s.skip = ws + o; o += up4(s.passes);
    s.words = o;
    return s;
}
uint64_t fr_sort_ws_words(uint64_t n, uint32_t n_keys) { return sort_ws(nullptr, n, n_keys).words; }
uint32_t fr_sort_tile() { return SORT_TILE; }

const uint32_t* launch_sort_front(hipStream_t s, const uint32_t* ev, uint64_t T, uint64_t n, uint32_t n_keys, uint32_t* keys,
                                  uint32_t* ws) {
    const SortWs W = sort_ws(ws, n, n_keys);
    (void)hipMemsetAsync(W.hist, 0, (size_t)W.passes * 256 * 4, s);
    const uint32_t bx = nblk(n, 256) < SORT_KEY_BLOCKS ? nblk(n, 256) : SORT_KEY_BLOCKS;
    k_sort_keys<<<dim3(bx, n_keys), 256, 0, s>>>(ev, keys, T, (uint32_t)n, n_keys, W.hist);
    k_sort_plan<<<W.passes, 256, 0, s>>>(W.hist, (uint32_t)n, W.skip);
    return W.skip;
}
const uint32_t* launch_sort_passes(hipStream_t s, const uint32_t* keys, uint64_t T, uint64_t n, uint32_t n_keys,
                                   const uint32_t* skip_host, uint32_t* ws) {
    const SortWs W = sort_ws(ws, n, n_keys);
    const uint32_t* cur = nullptr;
    int next = 0;
    for (uint32_t p = 0; p < W.passes; p++) {
        if (skip_host[p]) continue;
        const uint32_t c = n_keys - 1 - p / 32, b = p % 32;
        k_sort_count<<<W.ntiles, 256, 0, s>>>(keys, (uint64_t)c * T * 8 + (b >> 2), 8 * (b & 3), cur, (uint32_t)n, W.digit,
                                              W.tile_cnt, W.ntiles);
        k_sort_offsets<<<256, 256, 0, s>>>(W.tile_cnt, W.ntiles, W.hist + (uint64_t)p * 256);
        k_sort_scatter<<<W.ntiles, 256, 0, s>>>(W.digit, cur, W.perm[next], (uint32_t)n, W.tile_cnt, W.ntiles);
        cur = W.perm[next];
        next ^= 1;
    }
    return cur;
}
void launch_sort_gather(hipStream_t s, const uint32_t* col, const uint32_t* perm, uint32_t* out, uint64_t n) {
    if (n) k_sort_gather<<<nblk(n, 256), 256, 0, s>>>(col, perm, out, (uint32_t)n);
}
void launch_sort_tail(hipStream_t s, uint32_t* v, uint64_t n, uint64_t usable, const uint8_t* tail_be32, uint32_t* bad) {
    if (usable >= n || n - usable > BLIND_MAX_ROWS) return;
    SortTail tail;
    memset(&tail, 0, sizeof(tail));
    memcpy(tail.v, tail_be32, 32 * (size_t)(n - usable));
    k_sort_tail<<<1, 64, 0, s>>>(v, usable, (uint32_t)(n - usable), tail, bad);
}
