// fr_int.hip -- Fr-side kernels, part 13: the integer ALU columns of kzg_rows_commit_int.  Every output cell is a pure function
// of the CANONICAL INTEGERS of one or two source cells, each reduced to its low w bits (1 <= w <= 64, M = 2^w): and / or / xor,
// add with its carry, sub with its borrow, the low and high word of a product, quotient and remainder, and the two halves of
// a cell cut at a shift s.  A source column lies as an evaluation vector (T elements of 8 words, Montgomery, CANONICAL); rows
// [0, n) are read, n = usable (T in the plain layout); the rows behind are the caller's tail (launch_sort_tail).
//   ONE launch per call: grid (blocks over n, n_ops), 256 lanes per workgroup, one lane per cell.  The op table rides in the
//   kernel argument (48 B per op), so kind, width, count and the row pointers are scalar loads and every branch on them is
//   uniform over the workgroup.  A lane loads each DISTINCT operand in two 16-byte loads (one row may serve as both), takes its
//   canonical integer with fr9_from_mont (one product by 1), tests the words above bit w, and computes in uint64_t: the high
//   product is __umul64hi, every shift count of 64 is guarded, the divisor is replaced by 1 before the (software) division, so
//   b = 0, s = 0, s = w and w = 64 meet no undefined behaviour.  Each output is encoded with fr9_mont_from_u64 (a product of
//   radix 2^87) and fr9_canon, as k_fr_from_typed does, and stored in two 16-byte vector stores, lanes side by side.
//   Operand classes (fr29.hip.h): a loaded cell is canonical, a legal first operand of fr9_from_mont; fr9_mont_from_u64 leaves
//   an N-class value, which fr9_canon makes canonical.
//   A cell with an operand at or above 2^w (a SPLIT's shift cell: above w) is counted ONCE through derive_count (ballot ->
//   LDS -> one global add per workgroup); the first such row through expr_first (one 64-bit atomicMin per workgroup that has a
//   flagged lane).  Lanes t >= n read nothing and store nothing; they still walk the two reductions.
// Bound: 32 (operands + outputs) B of traffic per cell against one or two products by 1 and one or two short products; a
// DIVMOD adds the 64-bit software division.
#include <cstring>

#include "../../include/kzg_mi355x.h"   // the KZG_INT_* kinds
#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// (int_load and int_store, a cell's canonical integer in and a machine word out, live in fr_u64.hip.h: fr_alu.hip uses them too)

__global__ void __launch_bounds__(256) k_fr_int(const IntTab tab, uint64_t T, uint64_t n, unsigned long long* __restrict__ counts,
                                                 unsigned long long* __restrict__ first) {
    const IntOp& op = tab.op[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool over = false;
    if (t < n) {
        const uint32_t w = op.w;
        const uint64_t mask = w == 64 ? ~0ull : (1ull << w) - 1;
        bool ha, hb = false;
        const uint64_t ra = int_load(op.a + t * 8, &ha);
        uint64_t rb = op.imm;
        if (op.b == op.a) {
            rb = ra;
            hb = ha;
        } else if (op.b) {
            rb = int_load(op.b + t * 8, &hb);
        }
        const uint64_t a = ra & mask;
        over = ha || a != ra;
        uint64_t b, r0, r1;
        if (op.kind == KZG_INT_SPLIT) {   // the second operand is a shift in [0, w]
            b = hb || rb > w ? w : rb;
            over |= b != rb || hb;
        } else {
            b = rb & mask;
            over |= hb || b != rb;
        }
        switch (op.kind) {
            case KZG_INT_AND: r0 = a & b; r1 = 0; break;
            case KZG_INT_OR: r0 = a | b; r1 = 0; break;
            case KZG_INT_XOR: r0 = a ^ b; r1 = 0; break;
            case KZG_INT_ADD: {
                const uint64_t s = a + b;   // (below 2^64 when w < 64)
                r0 = s & mask;
                r1 = w == 64 ? (uint64_t)(s < a) : s >> w;
                break;
            }
            case KZG_INT_SUB: r0 = (a - b) & mask; r1 = a < b; break;
            case KZG_INT_MUL: {
                const uint64_t lo = a * b, hi = __umul64hi(a, b);
                r0 = lo & mask;
                r1 = w == 64 ? hi : (lo >> w) | (hi << (64 - w));   // (a b < 2^(2 w): nothing of hi is lost)
                break;
            }
            case KZG_INT_DIVMOD: {
                const uint64_t d = b ? b : 1, q = a / d;
                r0 = b ? q : mask;
                r1 = b ? a - q * d : a;
                break;
            }
            default:   // KZG_INT_SPLIT
                r0 = b >= 64 ? 0 : a >> b;
                r1 = b >= 64 ? a : a & ((1ull << b) - 1);
                break;
        }
        int_store(op.out + t * 8, r0);
        if (op.count == 2) int_store(op.out + (T + t) * 8, r1);
    }
    derive_count(over, counts + blockIdx.y);
    expr_first(over, first + blockIdx.y);
}

void launch_int(hipStream_t s, const IntTab& tab, uint32_t n_ops, uint64_t T, uint64_t n, uint64_t* counts, uint64_t* first) {
    if (!n || n > T || n_ops == 0 || n_ops > INT_MAX_OPS) return;
    for (uint32_t o = 0; o < n_ops; o++) {
        const IntOp& op = tab.op[o];
        if (!op.a || !op.out || op.w == 0 || op.w > 64 || op.count == 0 || op.count > 2 || op.kind < KZG_INT_AND ||
            op.kind > KZG_INT_SPLIT)
            return;
    }
    k_fr_int<<<dim3(nblk(n, 256), n_ops), 256, 0, s>>>(tab, T, n, reinterpret_cast<unsigned long long*>(counts),
                                                       reinterpret_cast<unsigned long long*>(first));
}
