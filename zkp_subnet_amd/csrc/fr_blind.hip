// fr_blind.hip -- Fr-side kernels, part 7: the blinding rows of the kzg_rows_commit_*_zk builders.  With u = usable < T the
// first u rows carry the circuit, row u is the "last" row and rows u + 1 .. T - 1 hold the caller's random values.  Two
// launches of one wave each (T - u <= BLIND_MAX_ROWS) around the plain builders' kernels, which run unchanged over T:
//   k_blind_mask   in front of the scan: the per-row operands of rows >= u become the scan's neutral element (N = D = 1 for
//                  the grand product; P = 0, Q = 1 for the lookup sum), so that nothing of a padding row -- a zero denominator
//                  included -- reaches the product, the inversion or the sum, and every row >= u leaves the scan as `closing`
//   k_blind_tail   behind the scan: rows u + 1 .. T - 1 are overwritten with the tail in Montgomery form
// No product per element of the row: the masks cost one short launch, not a compare in the hot kernels.
#include <cstring>

#include "fr_kernels.hip.h"

// a[t] <- 1 (a_one) or 0, b[t] <- 1 for usable <= t < n (Montgomery, canonical)
__global__ void __launch_bounds__(64) k_blind_mask(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint64_t n,
                                                    uint64_t usable, int a_one) {
    const uint64_t t = usable + threadIdx.x;
    if (t >= n) return;
    fr9_t one, va;
    fr9_one(one);   // R mod r: canonical as it stands
    if (a_one) va = one;
    else fr9_zero(va);
    fr9_store(a + 8 * t, va);
    fr9_store(b + 8 * t, one);
}
void launch_blind_mask(hipStream_t s, uint32_t* a, bool a_one, uint32_t* b, uint64_t n, uint64_t usable) {
    if (usable < n && n - usable <= BLIND_MAX_ROWS) k_blind_mask<<<1, 64, 0, s>>>(a, b, n, usable, a_one ? 1 : 0);
}

// v[usable + 1 + j] <- tail[j] for j < n - usable - 1: the tail rides in the kernel argument (at most 31 x 32 bytes)
struct BlindTail {
    FrArg v[BLIND_MAX_ROWS - 1];
};
__global__ void __launch_bounds__(64) k_blind_tail(uint32_t* __restrict__ v, uint64_t n, uint64_t usable, const BlindTail tail,
                                                    uint32_t* __restrict__ bad) {
    const uint32_t j = threadIdx.x;
    if (j >= BLIND_MAX_ROWS - 1 || usable + 1 + j >= n) return;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(tail.v[j].w[7 - i]);
    if (fr_words_ge_r(w)) atomicOr(bad, 1u);
    fr9_t x;
    fr9_from_words(x, w);
    fr9_to_mont(x, x);
    fr9_store(v + 8 * (usable + 1 + j), x);
}
void launch_blind_tail(hipStream_t s, uint32_t* v, uint64_t n, uint64_t usable, const uint8_t* tail_be32, uint32_t* bad) {
    if (usable + 1 >= n || n - usable > BLIND_MAX_ROWS) return;
    BlindTail tail;
    memset(&tail, 0, sizeof(tail));
    memcpy(tail.v, tail_be32, 32 * (size_t)(n - usable - 1));
    k_blind_tail<<<1, 64, 0, s>>>(v, n, usable, tail, bad);
}
