// fr_derive.hip -- Fr-side kernels, part 9: the helper columns of kzg_rows_commit_derived, each a pure function of ONE resident
// column.  A source column lies as an evaluation vector (T elements of 8 words, Montgomery, CANONICAL: the forward transform
// ends in fr9_reduce and a set stores canonical coefficients, so the field's zero is eight zero words).  Rows [0, n) of a source
// are read, n = usable (T in the plain layout); the rows behind are the caller's tail (launch_sort_tail).
//   inv0 prepare : Q[t] = x[t], or Montgomery 1 where x[t] = 0 and on the rows >= n, for ALL inv0 ops of the call side by side
//                  (op j at Q + j T elements): the vector launch_fr_batch_inv inverts with its one fr9_inv, and whose zero flag
//                  can no longer be raised.  The zero cells are remembered in a bit mask (32 cells per u32 word, one word per
//                  half wave, max(T / 32, 1) words per op) and counted: one ballot per wave, one LDS add per wave, one global
//                  add per workgroup.
//   inv0 finish  : per op, behind the inversion: 0 under the mask (only those cells are written), and the optional bit row
//                  (Montgomery 1 under the mask, else 0).
//   limbs        : one lane per cell: the element's canonical integer (one Montgomery product by 1), its L limbs of b bits
//                  (a limb may straddle a word border) as Montgomery elements (one product by R^2 each) into L vectors, lanes
//                  side by side in every one of them; the cells with a bit at or above b L are counted like the zeros.
// Every store is a vector store.  Bounds: prepare moves 64 B per cell (+ 1 bit), finish reads 1 bit per cell and writes 32 B per
// zero cell (+ 32 B per cell for a bit row), limbs moves 32 (1 + L) B per cell for 1 + L products: HBM on paper, the
// multiplier in practice once L >= 4.
#include <cstring>

#include "fr_kernels.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// (derive_count, the workgroup's count of flagged lanes, lives in fr_kernels.hip.h: fr_expr.hip counts with it too)

// ------------------------------------------------------------------------------------------------ inverse-or-zero
// grid (blocks over T, n_inv): op j = blockIdx.y reads src[j] (two ops may name one vector) and adds to counts[slot[j]]
struct Inv0Arg {
    const uint32_t* src[POLY_MAX_ROWS];
    uint32_t slot[POLY_MAX_ROWS];
};
__global__ void __launch_bounds__(256) k_inv0_prepare(const Inv0Arg arg, uint32_t* __restrict__ Q, uint32_t* __restrict__ mask,
                                                       uint64_t T, uint64_t n, uint32_t mask_words,
                                                       unsigned long long* __restrict__ counts) {
    const uint32_t j = blockIdx.y;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool zero = false;
    if (t < T) {
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (t < n) {
            const uint4* q = reinterpret_cast<const uint4*>(arg.src[j] + t * 8);
            a = q[0];
            b = q[1];
            zero = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
        }
        if (zero || t >= n) {
            fr9_t one;
            fr9_one(one);
            fr9_store(Q + ((uint64_t)j * T + t) * 8, one);
        } else {
            uint4* o = reinterpret_cast<uint4*>(Q + ((uint64_t)j * T + t) * 8);
            o[0] = a;
            o[1] = b;
        }
    }
    const unsigned long long bal = __ballot(zero);
    if (t < T && (threadIdx.x & 31u) == 0)
        mask[(uint64_t)j * mask_words + (t >> 5)] = (uint32_t)(bal >> (threadIdx.x & 32u));
    derive_count(zero, counts + arg.slot[j]);
}
// one op: inv[t] <- 0 where the mask says x[t] = 0; bit (null: no bit row) <- Montgomery 1 there, 0 elsewhere
__global__ void __launch_bounds__(256) k_inv0_finish(uint32_t* __restrict__ inv, const uint32_t* __restrict__ mask, uint64_t T,
                                                      uint32_t* __restrict__ bit) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const bool zero = (mask[t >> 5] >> (t & 31u)) & 1u;
    fr9_t z, one;
    fr9_zero(z);
    fr9_one(one);
    if (zero) fr9_store(inv + t * 8, z);
    if (bit) fr9_store(bit + t * 8, zero ? one : z);
}

// ------------------------------------------------------------------------------------------------ limbs
// w[i] for a run-time i < 8, without a run-time index into the registers
KZG_DEV uint32_t derive_word(const uint32_t* w, uint32_t i) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) r = i == k ? w[k] : r;
    return r;
}
// One lane per cell t < n.  Operand classes (fr29.hip.h): the loaded element is canonical, a legal first operand of
// fr9_from_mont, which leaves the canonical integer; a limb is an integer below 2^32 on two normalised 29-bit limbs, a legal
// first operand of fr9_to_mont, which leaves it canonical.  1 <= b <= 32, 1 <= L, b L <= 256.
__global__ void __launch_bounds__(256) k_limbs(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint64_t T, uint64_t n,
                                                uint32_t b, uint32_t L, unsigned long long* __restrict__ count) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool over = false;
    if (t < n) {
        uint32_t w[8];
        fr9_t v;
        fr9_load(v, src + t * 8);
        fr9_from_mont(v, v);
        fr9_to_words(w, v);
        const uint32_t top = b * L, tw = top >> 5, ts = top & 31u;   // the first bit no limb covers (256: none)
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) over |= k > tw ? w[k] != 0 : (k == tw && (w[k] >> ts) != 0);
        const uint32_t lmask = b == 32 ? 0xffffffffu : (1u << b) - 1u;
#pragma unroll 1
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t bit0 = b * l, wi = bit0 >> 5, sh = bit0 & 31u;
            const uint64_t two = ((uint64_t)(wi + 1 < 8 ? derive_word(w, wi + 1) : 0u) << 32) | derive_word(w, wi);
            const uint32_t limb = (uint32_t)(two >> sh) & lmask;
            fr9_t e;
            fr9_zero(e);
            e.l[0] = limb & FR9_MASK;
            e.l[1] = limb >> 29;
            fr9_to_mont(e, e);
            fr9_store(out + ((uint64_t)l * T + t) * 8, e);
        }
    }
    derive_count(over, count);
}

// ------------------------------------------------------------------------------------------------ launchers
uint32_t inv0_mask_words(uint64_t T) { return T < 32 ? 1u : (uint32_t)(T >> 5); }

void launch_inv0_prepare(hipStream_t s, const RowTab& src, const uint32_t* slot, uint32_t n_inv, uint32_t* Q, uint32_t* mask,
                         uint64_t T, uint64_t n, uint64_t* counts) {
    if (!T || !n_inv || n_inv > POLY_MAX_ROWS) return;
    Inv0Arg arg;
    memset(&arg, 0, sizeof(arg));
    for (uint32_t j = 0; j < n_inv; j++) {
        arg.src[j] = src.r[j];
        arg.slot[j] = slot[j];
    }
    k_inv0_prepare<<<dim3(nblk(T, 256), n_inv), 256, 0, s>>>(arg, Q, mask, T, n, inv0_mask_words(T),
                                                             reinterpret_cast<unsigned long long*>(counts));
}
void launch_inv0_finish(hipStream_t s, uint32_t* inv, const uint32_t* mask, uint64_t T, uint32_t* bit_or_null) {
    if (T) k_inv0_finish<<<nblk(T, 256), 256, 0, s>>>(inv, mask, T, bit_or_null);
}
void launch_limbs(hipStream_t s, const uint32_t* src, uint32_t* out, uint64_t T, uint64_t n, uint32_t bits, uint32_t count,
                  uint64_t* over) {
    if (!n || n > T || bits == 0 || bits > 32 || count == 0 || (uint64_t)bits * count > 256) return;
    k_limbs<<<nblk(n, 256), 256, 0, s>>>(src, out, T, n, bits, count, reinterpret_cast<unsigned long long*>(over));
}
