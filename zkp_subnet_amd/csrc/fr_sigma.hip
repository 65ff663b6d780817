// fr_sigma.hip -- Fr-side kernels, part 9: the permutation's sigma columns from variable labels (kzg_rows_commit_sigma) and the
// cell-by-cell check of copy constraints (kzg_rows_check_copies).  The k label columns lie as ONE vector of N = k n canonical
// Montgomery elements in flat-index order (cell j = c n + t: column c, row t < n), which the unchanged sort of fr_sort.hip
// orders with n_keys = 1: `keys` holds the cells' canonical integers (8 words each, by cell), `perm` the cells in sorted order
// (null: the identity -- no radix pass moved anything, e.g. every label equal).  The sort is stable, so a class (a run of equal
// keys) lies in ascending flat index and its first position is the class's smallest cell.
//   link     : one lane per sorted position p.  Its cell maps to the cell of p + 1, or at a run's end to the run's first
//              position, found by a bounded binary search (the lower bound of the key over positions [0, p], at most 27
//              steps: one label may fill the whole vector, so nothing walks backwards).  A cell that carries the free label
//              maps to itself.  The lane writes sigma_c(w^t) = shift[c'] w^t' of its image (c', t') and counts the run ends
//              (one per class) and the self-mapped cells
//   identity : rows t >= n of every column: sigma_c(w^t) = shift[c] w^t
//   check    : one lane per sorted position: the cell's wire value against that of its run's first position (canonical
//              Montgomery words compare like the values they stand for), counted, with the smallest violating flat index
// w^t' comes from the resident forward twiddle table as in k_gp_factors: T / 2 nine-limb slots of 48 bytes, w^(t + T/2) = -w^t,
// unused at T = 1.  The shifts and the free label ride as kernel arguments.  Bounds: link is one Montgomery product per cell
// plus the gathers keys[perm[p + 1]] (32 bytes, uncoalesced) and, at run ends, up to 27 dependent gathers keys[perm[mid]];
// check takes that search at every position.  The counts are sums and a minimum: no result depends on the order of an atomic.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

struct SigmaArg {
    FrArg shift[SIGMA_MAX_COLS];
    FrArg free_label;
};

// the canonical integer of cell j: 8 little-endian words, two 16-byte loads
KZG_DEV void sigma_key(uint32_t* w, const uint32_t* __restrict__ keys, uint32_t j) {
    const uint4* q = reinterpret_cast<const uint4*>(keys + (uint64_t)j * 8);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
KZG_DEV bool sigma_same(const uint32_t* a, const uint32_t* b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
    return d == 0;
}
KZG_DEV bool sigma_less(const uint32_t* a, const uint32_t* b) {   // a < b as 256-bit integers
    bool lt = false;
#pragma unroll
    for (int i = 0; i < 8; i++) lt = a[i] < b[i] || (a[i] == b[i] && lt);   // the most significant word decides last
    return lt;
}
KZG_DEV uint32_t sigma_cell(const uint32_t* __restrict__ perm, uint32_t p) { return perm ? perm[p] : p; }
// the first sorted position whose key is `key`, which position p holds: the lower bound over [0, p].  p < 2^27: 27 halvings
KZG_DEV uint32_t sigma_run_head(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, uint32_t p,
                                const uint32_t* key) {
    uint32_t lo = 0, hi = p;
    for (int step = 0; step < 27 && lo < hi; step++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t km[8];
        sigma_key(km, keys, sigma_cell(perm, mid));
        if (sigma_less(km, key)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
KZG_DEV void sigma_arg_words(uint32_t* w, const FrArg& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(a.w[7 - i]);
}
// the shifts into LDS as canonical Montgomery limbs, one lane each; workgroup 0 raises *bad for a shift >= r
KZG_DEV void sigma_shifts(uint32_t (*sh)[9], const SigmaArg& arg, uint32_t k, uint32_t* __restrict__ bad) {
    const uint32_t v = threadIdx.x;
    if (v < k && v < SIGMA_MAX_COLS) {
        uint32_t w[8];
        sigma_arg_words(w, arg.shift[v]);
        if (blockIdx.x == 0 && blockIdx.y == 0 && fr_words_ge_r(w)) atomicOr(bad, 1u);
        fr9_t s;
        fr9_from_words(s, w);
        fr9_to_mont(s, s);
#pragma unroll
        for (int i = 0; i < 9; i++) sh[v][i] = s.l[i];
    }
    __syncthreads();
}
// sig[c T + t] <- shift[ci] w^ti, canonical.  Operand classes (fr29.hip.h): the shift is canonical, a legal first operand; the
// twiddle is normalised; the product is class N (< 2r); 4r - x is lazy (< 4r), which fr9_reduce takes
KZG_DEV void sigma_store(uint32_t* __restrict__ sig, uint64_t T, uint32_t c, uint64_t t, uint32_t ci, uint64_t ti,
                         const uint32_t* __restrict__ tw, const uint32_t (*sh)[9]) {
    fr9_t s, x;
#pragma unroll
    for (int i = 0; i < 9; i++) s.l[i] = sh[ci][i];
    const uint64_t half = T >> 1;
    if (half) {
        fr9_t w;
        const uint4* q = reinterpret_cast<const uint4*>(tw + 12 * (ti & (half - 1)));
        const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
        w.l[0] = q0.x; w.l[1] = q0.y; w.l[2] = q0.z; w.l[3] = q0.w;
        w.l[4] = q1.x; w.l[5] = q1.y; w.l[6] = q1.z; w.l[7] = q1.w;
        w.l[8] = q2.x;
        fr9_mul(x, s, w);
        if (ti >= half) {                         // w^ti = -w^(ti - T/2)
            fr9_t z;
            fr9_zero(z);
            fr9_sub4(x, z, x);
            fr9_reduce(x, x);
        } else {
            fr9_canon(x, x);
        }
    } else {
        x = s;                                    // T == 1: w^0 = 1
    }
    fr9_store(sig + ((uint64_t)c * T + t) * 8, x);
}

// ------------------------------------------------------------------------------------------------ link
// grid = N / 256 positions.  stats[0] += run ends of non-free keys (the classes), stats[1] += cells that map to themselves
__global__ void __launch_bounds__(256) k_sigma_link(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                     uint32_t N, uint32_t n, uint64_t T, uint32_t k,
                                                     const uint32_t* __restrict__ tw, const SigmaArg arg, uint32_t has_free,
                                                     uint32_t* __restrict__ sig, unsigned long long* __restrict__ stats,
                                                     uint32_t* __restrict__ bad) {
    __shared__ uint32_t sh[SIGMA_MAX_COLS][9];
    sigma_shifts(sh, arg, k, bad);
    if (has_free && blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t fw[8];
        sigma_arg_words(fw, arg.free_label);
        if (fr_words_ge_r(fw)) atomicOr(bad, 1u);
    }
    const uint64_t p64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool cls = false, fix = false;
    if (p64 < N) {
        const uint32_t p = (uint32_t)p64, j = sigma_cell(perm, p);
        uint32_t key[8], other[8];
        sigma_key(key, keys, j);
        bool free_cell = false;
        if (has_free) {
            sigma_arg_words(other, arg.free_label);
            free_cell = sigma_same(key, other);
        }
        bool end = true;
        uint32_t img = 0;
        if (p + 1 < N) {
            img = sigma_cell(perm, p + 1);
            sigma_key(other, keys, img);
            end = !sigma_same(key, other);
        }
        if (free_cell) img = j;
        else if (end) img = sigma_cell(perm, sigma_run_head(keys, perm, p, key));
        cls = end && !free_cell;
        fix = img == j;
        const uint32_t c = j / n, ci = img / n;
        sigma_store(sig, T, c, j - c * n, ci, img - ci * n, tw, sh);
    }
    derive_count(cls, stats);
    derive_count(fix, stats + 1);
}
// grid (rows [n, T) / 256, k): the cells that take no part map to themselves
__global__ void __launch_bounds__(256) k_sigma_identity(uint64_t n, uint64_t T, uint32_t k, const uint32_t* __restrict__ tw,
                                                         const SigmaArg arg, uint32_t* __restrict__ sig,
                                                         uint32_t* __restrict__ bad) {
    __shared__ uint32_t sh[SIGMA_MAX_COLS][9];
    sigma_shifts(sh, arg, k, bad);
    const uint64_t t = n + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (t < T && c < k) sigma_store(sig, T, c, t, c, t, tw, sh);
}

// ------------------------------------------------------------------------------------------------ check
// grid = N / 256 positions.  wires.r[c]: column c as T canonical Montgomery elements.  out[0] += violations, out[1] <- min(out[1],
// the smallest violating flat index c T + t).  One LDS minimum per violating lane (rare), one global pair per workgroup
__global__ void __launch_bounds__(256) k_copy_check(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, uint32_t N,
                                                     uint32_t n, uint64_t T, const RowTab wires, const SigmaArg arg,
                                                     uint32_t has_free, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long wg_first;
    if (threadIdx.x == 0) wg_first = ~0ull;
    __syncthreads();
    const uint64_t p64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool viol = false;
    if (p64 < N) {
        const uint32_t p = (uint32_t)p64, j = sigma_cell(perm, p);
        uint32_t key[8], other[8];
        sigma_key(key, keys, j);
        bool free_cell = false;
        if (has_free) {
            sigma_arg_words(other, arg.free_label);
            free_cell = sigma_same(key, other);
        }
        if (!free_cell) {
            const uint32_t jh = sigma_cell(perm, sigma_run_head(keys, perm, p, key));
            if (jh != j) {
                const uint32_t c = j / n, ch = jh / n;
                const uint32_t t = j - c * n, th = jh - ch * n;
                sigma_key(key, wires.r[c], t);
                sigma_key(other, wires.r[ch], th);
                viol = !sigma_same(key, other);
                if (viol) atomicMin(&wg_first, (unsigned long long)c * T + t);
            }
        }
    }
    derive_count(viol, out);      // (its barriers order the LDS minima before the read below)
    if (threadIdx.x == 0 && wg_first != ~0ull) atomicMin(out + 1, wg_first);
}

// ------------------------------------------------------------------------------------------------ launchers
static bool sigma_shape_ok(uint64_t N, uint64_t n, uint64_t T, uint32_t k) {
    return k >= 1 && k <= SIGMA_MAX_COLS && n >= 1 && n <= T && N == (uint64_t)k * n && N <= ((uint64_t)1 << 27);
}
static SigmaArg sigma_arg(const uint8_t* shifts_be32, uint32_t k, const uint8_t* free_be32) {
    SigmaArg arg;
    memset(&arg, 0, sizeof(arg));
    if (shifts_be32) memcpy(arg.shift, shifts_be32, 32 * (size_t)k);
    if (free_be32) memcpy(arg.free_label.w, free_be32, 32);
    return arg;
}
void launch_sigma_link(hipStream_t s, const uint32_t* keys, const uint32_t* perm, uint64_t N, uint64_t n, uint64_t T, uint32_t k,
                       const uint32_t* tw, const uint8_t* shifts_be32, const uint8_t* free_be32, uint32_t* sig, uint64_t* stats,
                       uint32_t* bad) {
    if (!sigma_shape_ok(N, n, T, k)) return;
    k_sigma_link<<<nblk(N, 256), 256, 0, s>>>(keys, perm, (uint32_t)N, (uint32_t)n, T, k, tw, sigma_arg(shifts_be32, k, free_be32),
                                               free_be32 ? 1u : 0u, sig, reinterpret_cast<unsigned long long*>(stats), bad);
}
void launch_sigma_identity(hipStream_t s, uint64_t n, uint64_t T, uint32_t k, const uint32_t* tw, const uint8_t* shifts_be32,
                           uint32_t* sig, uint32_t* bad) {
    if (k < 1 || k > SIGMA_MAX_COLS || n >= T) return;
    k_sigma_identity<<<dim3(nblk(T - n, 256), k), 256, 0, s>>>(n, T, k, tw, sigma_arg(shifts_be32, k, nullptr), sig, bad);
}
void launch_copy_check(hipStream_t s, const uint32_t* keys, const uint32_t* perm, uint64_t N, uint64_t n, uint64_t T, uint32_t k,
                       const RowTab& wires, const uint8_t* free_be32, uint64_t* out) {
    if (!sigma_shape_ok(N, n, T, k)) return;
    k_copy_check<<<nblk(N, 256), 256, 0, s>>>(keys, perm, (uint32_t)N, (uint32_t)n, T, wires, sigma_arg(nullptr, k, free_be32),
                                               free_be32 ? 1u : 0u, reinterpret_cast<unsigned long long*>(out));
}
