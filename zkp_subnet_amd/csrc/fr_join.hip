// fr_join.hip -- Fr-side kernels, part 6: the hash join of kzg_rows_commit_multiplicities.  The w table columns and the w
// columns of one lookup lie as evaluation vectors (T elements of 8 words, Montgomery, CANONICAL: the forward transform ends
// in fr9_reduce and a set stores canonical coefficients, so equal field elements are equal words and the join compares and
// hashes words).  Column c of a tuple is cols + c * T * 8 words.
//   build : slot[hash(tab(t)) ...] <- the SMALLEST t with that tuple              (open addressing, linear probing)
//   probe : cnt[first(in(l, t))] += 1, or missing += 1                            (one launch per lookup)
//           (_sel: only where the lookup's selector q_l(w^t) is not zero)
//   counts: cnt[t] -> m(w^t) as a Montgomery element
//   fetch : out[p][t] <- tab[n_keys + p][first(in(l, t))], or 0 and missing += 1    (kzg_rows_commit_fetch; one launch per read;
//           k_fetch_index: the row is the cell's canonical integer instead of a walk)
// A slot holds a table ROW INDEX or JOIN_EMPTY = 2^32 - 1 (T <= 2^27, so 0 and T - 1 are ordinary values).  No kernel here
// multiplies (the last one: one product per element); they move bytes and chase one dependent load (slot -> row).
#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

#define JOIN_EMPTY 0xffffffffu

// murmur3's 32-bit block step and finaliser over all w * 8 words: every input bit reaches every bit of the slot index, so
// keys that differ in one limb or in the last column only spread like random ones
KZG_DEV uint32_t join_mix(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = (k << 15) | (k >> 17);
    k *= 0x1b873593u;
    h ^= k;
    h = (h << 13) | (h >> 19);
    return h * 5u + 0xe6546b64u;
}
KZG_DEV uint32_t join_fmix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}
// the hash of the w * 32 bytes of tuple t
KZG_DEV uint32_t join_hash(const uint32_t* __restrict__ cols, uint64_t T, uint32_t w, uint64_t t) {
    uint32_t h = 0x9747b28cu;
    for (uint32_t c = 0; c < w; c++) {
        const uint4* q = reinterpret_cast<const uint4*>(cols + ((uint64_t)c * T + t) * 8);
        const uint4 a = q[0], b = q[1];
        h = join_mix(h, a.x); h = join_mix(h, a.y); h = join_mix(h, a.z); h = join_mix(h, a.w);
        h = join_mix(h, b.x); h = join_mix(h, b.y); h = join_mix(h, b.z); h = join_mix(h, b.w);
    }
    return join_fmix(h ^ (w * 32u));
}
// tuple ta of A == tuple tb of B, in ALL w columns (stops at the first column that differs)
KZG_DEV bool join_equal(const uint32_t* __restrict__ A, uint64_t ta, const uint32_t* __restrict__ B, uint64_t tb, uint64_t T,
                        uint32_t w) {
    for (uint32_t c = 0; c < w; c++) {
        const uint4* p = reinterpret_cast<const uint4*>(A + ((uint64_t)c * T + ta) * 8);
        const uint4* q = reinterpret_cast<const uint4*>(B + ((uint64_t)c * T + tb) * 8);
        const uint4 a0 = p[0], a1 = p[1], b0 = q[0], b1 = q[1];
        const uint32_t d = (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) |
                           (a1.z ^ b1.z) | (a1.w ^ b1.w);
        if (d) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ build
// One lane per table row t.  The lane walks its probe sequence; an EMPTY slot is claimed with atomicCAS; an occupied slot
// names a row q of the table, whose columns were complete before the launch: if tab(q) == tab(t) the slot is this tuple's
// and takes min(slot, t), else the walk goes on.  A claimed slot never becomes empty and only ever holds rows of ONE tuple
// (a lane writes its index only into an empty slot or into a slot whose row it has compared equal), so two lanes with one
// tuple stop at the same slot and the slot ends at the smallest index whatever the schedule.  Wait-free: no lane waits for
// another lane's write.  The walk is bounded by the capacity (cap = mask + 1 >= 2 T slots and at most T tuples, so an empty
// slot always exists); a lane that reaches the bound raises *overrun.
__global__ void __launch_bounds__(256) k_join_build(const uint32_t* __restrict__ tab, uint64_t T, uint32_t w, uint32_t* slots,
                                                     uint32_t mask, uint32_t* overrun) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    uint32_t s = join_hash(tab, T, w, t) & mask;
    for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(slots + s, JOIN_EMPTY, (uint32_t)t);
        if (cur == JOIN_EMPTY) return;
        if (cur < T && join_equal(tab, cur, tab, t, T, w)) {
            atomicMin(slots + s, (uint32_t)t);
            return;
        }
    }
    atomicOr(overrun, 1u);
}
// kzg_rows_commit_multiplicities_zk: the table's first `rows` rows only (the columns still lie T apart).  The same walk,
// kept as a kernel of its own so that the plain call's keeps its instructions.
__global__ void __launch_bounds__(256) k_join_build_rows(const uint32_t* __restrict__ tab, uint64_t T, uint64_t rows, uint32_t w,
                                                          uint32_t* slots, uint32_t mask, uint32_t* overrun) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    uint32_t s = join_hash(tab, T, w, t) & mask;
    for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(slots + s, JOIN_EMPTY, (uint32_t)t);
        if (cur == JOIN_EMPTY) return;
        if (cur < T && join_equal(tab, cur, tab, t, T, w)) {
            atomicMin(slots + s, (uint32_t)t);
            return;
        }
    }
    atomicOr(overrun, 1u);
}

// ------------------------------------------------------------------------------------------------ probe
// One lane per cell t of one lookup.  The walk of the build: an empty slot ends it with a miss; a slot whose row equals the
// cell's tuple in all w columns ends it with one atomicAdd to that row's counter (the slot holds first(tuple): the build
// has finished).  The misses of a workgroup are counted in LDS (one ballot per wave) and leave it as ONE atomic.
__global__ void __launch_bounds__(256) k_join_probe(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ in, uint64_t T,
                                                     uint32_t w, const uint32_t* __restrict__ slots, uint32_t mask,
                                                     uint32_t* cnt, unsigned long long* missing, uint32_t* overrun) {
    __shared__ uint32_t wg_miss;
    if (threadIdx.x == 0) wg_miss = 0;
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (t < T) {
        uint32_t s = join_hash(in, T, w, t) & mask;
        bool done = false;
        for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
            const uint32_t q = slots[s];
            if (q == JOIN_EMPTY) { miss = done = true; break; }
            if (q < T && join_equal(tab, q, in, t, T, w)) {
                atomicAdd(cnt + q, 1u);
                done = true;
                break;
            }
        }
        if (!done) atomicOr(overrun, 1u);
    }
    const unsigned long long b = __ballot(miss);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&wg_miss, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && wg_miss) atomicAdd(missing, (unsigned long long)wg_miss);
}
// kzg_rows_commit_multiplicities_zk: one lookup's first `rows` cells only (a kernel of its own, as for the build)
__global__ void __launch_bounds__(256) k_join_probe_rows(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ in,
                                                          uint64_t T, uint64_t rows, uint32_t w,
                                                          const uint32_t* __restrict__ slots, uint32_t mask, uint32_t* cnt,
                                                          unsigned long long* missing, uint32_t* overrun) {
    __shared__ uint32_t wg_miss;
    if (threadIdx.x == 0) wg_miss = 0;
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (t < rows) {
        uint32_t s = join_hash(in, T, w, t) & mask;
        bool done = false;
        for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
            const uint32_t q = slots[s];
            if (q == JOIN_EMPTY) { miss = done = true; break; }
            if (q < T && join_equal(tab, q, in, t, T, w)) {
                atomicAdd(cnt + q, 1u);
                done = true;
                break;
            }
        }
        if (!done) atomicOr(overrun, 1u);
    }
    const unsigned long long b = __ballot(miss);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&wg_miss, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && wg_miss) atomicAdd(missing, (unsigned long long)wg_miss);
}

// kzg_rows_commit_multiplicities_sel: the probe of k_join_probe_rows for a lookup with a selector row.  sel holds q_l's T
// evaluations (canonical Montgomery words like the tuples: 0 is eight zero words): one more 32-byte load per cell, and a lane
// whose selector is zero neither walks nor counts a miss.  rows = T is the plain layout, rows = usable the _zk one.  A
// kernel of its own: the two probes above keep their instructions, and a lookup without a selector still launches them.
__global__ void __launch_bounds__(256) k_join_probe_sel(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ in,
                                                         const uint32_t* __restrict__ sel, uint64_t T, uint64_t rows, uint32_t w,
                                                         const uint32_t* __restrict__ slots, uint32_t mask, uint32_t* cnt,
                                                         unsigned long long* missing, uint32_t* overrun) {
    __shared__ uint32_t wg_miss;
    if (threadIdx.x == 0) wg_miss = 0;
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (t < rows) {
        const uint4* sq = reinterpret_cast<const uint4*>(sel + 8 * t);
        const uint4 s0 = sq[0], s1 = sq[1];
        if (s0.x | s0.y | s0.z | s0.w | s1.x | s1.y | s1.z | s1.w) {
            uint32_t s = join_hash(in, T, w, t) & mask;
            bool done = false;
            for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
                const uint32_t q = slots[s];
                if (q == JOIN_EMPTY) { miss = done = true; break; }
                if (q < T && join_equal(tab, q, in, t, T, w)) {
                    atomicAdd(cnt + q, 1u);
                    done = true;
                    break;
                }
            }
            if (!done) atomicOr(overrun, 1u);
        }
    }
    const unsigned long long b = __ballot(miss);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&wg_miss, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && wg_miss) atomicAdd(missing, (unsigned long long)wg_miss);
}

// ------------------------------------------------------------------------------------------------ counters -> Fr
// m(w^t) = cnt[t] as a canonical Montgomery element: what the inverse transform of row_to_coeffs reads
__global__ void __launch_bounds__(256) k_join_counts(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ out, uint64_t T) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    fr9_t v;
    fr9_zero(v);
    const uint32_t c = cnt[t];
    v.l[0] = c & FR9_MASK;
    v.l[1] = c >> 29;
    fr9_to_mont(v, v);
    fr9_store(out + 8 * t, v);
}

// ------------------------------------------------------------------------------------------------ fetch
// kzg_rows_commit_fetch: the probe that copies.  The misses of a workgroup and its smallest missing cell: one ballot per wave,
// an LDS sum and an LDS minimum (the lowest set bit of the ballot), one atomicAdd and one atomicMin on u64 words per workgroup
// -- a sum and a minimum of minima, whatever the order in which the atomics return.  Called by every lane of the workgroup
// (uniform control flow); lane v stands for cell blockIdx.x * blockDim.x + v
KZG_DEV void fetch_tally(bool miss, unsigned long long* __restrict__ missing, unsigned long long* __restrict__ first) {
    __shared__ uint32_t wg_miss, wg_first;
    if (threadIdx.x == 0) {
        wg_miss = 0;
        wg_first = 0xffffffffu;
    }
    __syncthreads();
    const unsigned long long b = __ballot(miss);
    if ((threadIdx.x & 63u) == 0 && b) {
        atomicAdd(&wg_miss, (uint32_t)__popcll(b));
        atomicMin(&wg_first, threadIdx.x + (uint32_t)__ffsll(b) - 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_miss) {
        atomicAdd(missing, (unsigned long long)wg_miss);
        atomicMin(first, (unsigned long long)blockIdx.x * blockDim.x + wg_first);
    }
}
// cell t of the n_out = index + n_pay output vectors (T elements apart) of one read: on a hit at table row q the index column
// (if any) takes q as a canonical Montgomery element, as k_join_counts converts a counter, and payload column p the 32 bytes of
// pay[p T + q] (two 16-byte loads, the gather; two 16-byte stores, coalesced); on a miss every column takes 0.  Vector stores only
KZG_DEV void fetch_emit(const uint32_t* __restrict__ pay, uint32_t* __restrict__ out, uint64_t T, uint64_t t, bool hit, uint32_t q,
                        uint32_t n_pay, bool index) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    if (index) {
        if (hit) {
            fr9_t v;
            fr9_zero(v);
            v.l[0] = q & FR9_MASK;
            v.l[1] = q >> 29;
            fr9_to_mont(v, v);
            fr9_store(out + 8 * t, v);
        } else {
            uint4* o = reinterpret_cast<uint4*>(out + 8 * t);
            o[0] = z;
            o[1] = z;
        }
        out += T * 8;
    }
    for (uint32_t p = 0; p < n_pay; p++) {
        uint4 a = z, b = z;
        if (hit) {
            const uint4* g = reinterpret_cast<const uint4*>(pay + ((uint64_t)p * T + q) * 8);
            a = g[0];
            b = g[1];
        }
        uint4* o = reinterpret_cast<uint4*>(out + ((uint64_t)p * T + t) * 8);
        o[0] = a;
        o[1] = b;
    }
}
// One lane per cell t < rows of one read; the walk of k_join_probe_rows over a join built on the table's first w = n_keys
// columns and its first `rows` rows (rows = T: all of them).  A slot's row q is below `rows` (the build wrote it), so every
// gather stays inside the table's vectors; the payload columns are the table's vectors n_keys .. n_keys + n_pay - 1.  A walk
// that reaches its bound raises *overrun and writes the zeros of a miss (the caller fails the call).  Lanes t >= rows read and
// store nothing; they still walk the reduction.
__global__ void __launch_bounds__(256) k_join_fetch(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ in, uint64_t T,
                                                     uint64_t rows, uint32_t w, uint32_t n_pay, uint32_t index,
                                                     const uint32_t* __restrict__ slots, uint32_t mask, uint32_t* __restrict__ out,
                                                     unsigned long long* __restrict__ missing,
                                                     unsigned long long* __restrict__ first, uint32_t* overrun) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (t < rows) {
        uint32_t s = join_hash(in, T, w, t) & mask, q = 0;
        bool hit = false, done = false;
        for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
            q = slots[s];
            if (q == JOIN_EMPTY) { miss = done = true; break; }
            if (q < rows && join_equal(tab, q, in, t, T, w)) { hit = done = true; break; }
        }
        if (!done) atomicOr(overrun, 1u);
        fetch_emit(tab + (uint64_t)w * T * 8, out, T, t, hit, q, n_pay, index != 0);
    }
    fetch_tally(miss, missing, first);
}
// n_keys = 0: the cell is the ADDRESS.  It is decoded from Montgomery form to its canonical integer as k_limbs decodes a cell;
// the range test reads all eight words (2^32 + 3 or 2^64 is a miss, not row 3 or row 0), so a hit's q is below rows <= T and
// every gather stays inside the table's vectors, which are all payload.
__global__ void __launch_bounds__(256) k_fetch_index(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ addr, uint64_t T,
                                                      uint64_t rows, uint32_t n_pay, uint32_t* __restrict__ out,
                                                      unsigned long long* __restrict__ missing,
                                                      unsigned long long* __restrict__ first) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (t < rows) {
        uint32_t w[8];
        fr9_t v;
        fr9_load(v, addr + t * 8);
        fr9_from_mont(v, v);
        fr9_to_words(w, v);
        const bool hit = (w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0 && w[0] < rows;
        miss = !hit;
        fetch_emit(tab, out, T, t, hit, hit ? w[0] : 0u, n_pay, false);
    }
    fetch_tally(miss, missing, first);
}

// test hook (kzg_test_join): the home slot of tuple t < n, the slot at which every walk above starts
__global__ void __launch_bounds__(256) k_join_home(const uint32_t* __restrict__ cols, uint64_t T, uint32_t w, uint64_t n,
                                                    uint32_t mask, uint32_t* __restrict__ home) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) home[t] = join_hash(cols, T, w, t) & mask;
}
void launch_join_home(hipStream_t s, const uint32_t* cols, uint64_t T, uint32_t w, uint64_t n, uint32_t cap, uint32_t* home) {
    if (n && n <= T) k_join_home<<<nblk(n, 256), 256, 0, s>>>(cols, T, w, n, cap - 1, home);
}

void launch_join_build(hipStream_t s, const uint32_t* tab, uint64_t T, uint32_t w, uint32_t* slots, uint32_t cap,
                       uint32_t* overrun) {
    if (T) k_join_build<<<nblk(T, 256), 256, 0, s>>>(tab, T, w, slots, cap - 1, overrun);
}
void launch_join_probe(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint32_t w, const uint32_t* slots,
                       uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun) {
    if (T)
        k_join_probe<<<nblk(T, 256), 256, 0, s>>>(tab, in, T, w, slots, cap - 1, cnt, reinterpret_cast<unsigned long long*>(missing),
                                                   overrun);
}
void launch_join_build_rows(hipStream_t s, const uint32_t* tab, uint64_t T, uint64_t rows, uint32_t w, uint32_t* slots,
                            uint32_t cap, uint32_t* overrun) {
    if (rows) k_join_build_rows<<<nblk(rows, 256), 256, 0, s>>>(tab, T, rows, w, slots, cap - 1, overrun);
}
void launch_join_probe_rows(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint64_t rows, uint32_t w,
                            const uint32_t* slots, uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun) {
    if (rows)
        k_join_probe_rows<<<nblk(rows, 256), 256, 0, s>>>(tab, in, T, rows, w, slots, cap - 1, cnt,
                                                           reinterpret_cast<unsigned long long*>(missing), overrun);
}
void launch_join_probe_sel(hipStream_t s, const uint32_t* tab, const uint32_t* in, const uint32_t* sel, uint64_t T, uint64_t rows,
                           uint32_t w, const uint32_t* slots, uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun) {
    if (rows)
        k_join_probe_sel<<<nblk(rows, 256), 256, 0, s>>>(tab, in, sel, T, rows, w, slots, cap - 1, cnt,
                                                          reinterpret_cast<unsigned long long*>(missing), overrun);
}
void launch_join_counts(hipStream_t s, const uint32_t* cnt, uint32_t* out, uint64_t T) {
    if (T) k_join_counts<<<nblk(T, 256), 256, 0, s>>>(cnt, out, T);
}
void launch_join_fetch(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint64_t rows, uint32_t n_keys,
                       uint32_t n_pay, bool index, const uint32_t* slots, uint32_t cap, uint32_t* out, uint64_t* missing,
                       uint64_t* first, uint32_t* overrun) {
    if (!rows || rows > T || T > ((uint64_t)1 << 27) || n_keys == 0 || (n_pay == 0 && !index)) return;
    k_join_fetch<<<nblk(rows, 256), 256, 0, s>>>(tab, in, T, rows, n_keys, n_pay, index ? 1u : 0u, slots, cap - 1, out,
                                                  reinterpret_cast<unsigned long long*>(missing),
                                                  reinterpret_cast<unsigned long long*>(first), overrun);
}
void launch_fetch_index(hipStream_t s, const uint32_t* tab, const uint32_t* addr, uint64_t T, uint64_t rows, uint32_t n_pay,
                        uint32_t* out, uint64_t* missing, uint64_t* first) {
    if (!rows || rows > T || T > ((uint64_t)1 << 27) || n_pay == 0) return;
    k_fetch_index<<<nblk(rows, 256), 256, 0, s>>>(tab, addr, T, rows, n_pay, out, reinterpret_cast<unsigned long long*>(missing),
                                                   reinterpret_cast<unsigned long long*>(first));
}
