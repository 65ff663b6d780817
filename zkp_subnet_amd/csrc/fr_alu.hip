// fr_alu.hip -- Fr-side kernels, part 14: the ALU column of kzg_rows_commit_alu, the machine-word arithmetic of fr_int.hip with
// the KIND CHOSEN PER CELL by an op-code column.  Cell t of a unit reads c, the canonical integer of op[t]; program entry c
// gives the kind (KZG_ALU_*), the width w (1 <= w <= 64, M = 2^w) and, optionally, an immediate second operand.  c at or
// beyond the program is UNKNOWN and an entry of kind 0 is IDLE: both write 0 into every output row and load neither operand.
//   ONE launch per call: grid (blocks over n, units), 256 lanes per workgroup, one lane per cell.  The units (their row pointers
//   and counts) ride in the kernel argument and are indexed by blockIdx.y: scalar loads, uniform branches, as in k_fr_int.
//   THE PROGRAM IS STAGED INTO LDS at workgroup start (lane e < n_prog copies entry e, 16 B; at most 1 KiB) and a lane fetches
//   its entry with one 16-byte LDS read.  k_fr_int indexes its table by blockIdx.y, this kernel by a per-lane value: indexing
//   the kernel argument itself per lane would be a vector load from the argument segment per cell (or, where the compiler
//   copies the by-value struct, 1 KiB of scratch per lane); the LDS copy is loaded once per workgroup and costs no scratch.
//   The kind diverges inside a wave, so the arithmetic is FOUR SHARED CORES, each computed once per lane whatever the kinds
//   present, and a per-kind select of their results:
//     add / sub / compare   a + b, a - b, a < b unsigned and (through the flipped sign bit) signed, a = b
//     product               ONE 64 x 64 -> 128 product; the signed high words subtract b where a < 0 and a where b < 0
//     division              ONE software division q = num / den: magnitudes for DIV and REM with the sign fix-up behind it,
//                           the operands themselves for DIVMOD and REMU, and (b, w) for a shift kind at a width that is no
//                           power of two, whose amount is b mod w.  Waves without such a lane skip it; a divergent wave
//                           runs it once, not once per kind.  A zero divisor is replaced by 1 before the division
//     shift                 a >> s, a mod 2^s, a << s, the top s bits, for s in [0, 64]: SPLIT, the five shifts and
//                           rotations, and SEXT (s = the field width f)
//   Every shift count of 64 is guarded or masked (s = 0, s = w, w - s = w, w = 64 meet no undefined behaviour), w = 1 runs
//   the same code (sgn 1 = -1, s = 0).  Loading and storing are int_load / int_store of fr_u64.hip.h: two 16-byte loads per
//   distinct operand (one row may serve as op, a and b), two 16-byte VECTOR stores per output cell.
//   A cell with an operand out of range is counted ONCE through derive_count and the first such row found through expr_first
//   (fr_kernels.hip.h); the unknown cells are a second pair of the same reductions.  Lanes t >= n read nothing and store
//   nothing; they still walk the four reductions.
// Bound: 32 B read per distinct operand and written per output row of a cell, against three products by 1, two short products
// and a few dozen 64-bit integer ops; a dividing or odd-width shifting wave adds one 64-bit software division.
#include "../../include/kzg_mi355x.h"   // the KZG_ALU_* kinds
#include "fr_kernels.hip.h"
#include "fr_u64.hip.h"

static inline uint32_t nblk(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

__global__ void __launch_bounds__(256) k_fr_alu(const AluTab tab, uint32_t n_prog, uint64_t T, uint64_t n,
                                                 unsigned long long* __restrict__ counts, unsigned long long* __restrict__ unknown,
                                                 unsigned long long* __restrict__ first, unsigned long long* __restrict__ first_unknown) {
    __shared__ __align__(16) AluEnt prog[ALU_MAX_PROG];
    if (threadIdx.x < n_prog) prog[threadIdx.x] = tab.prog[threadIdx.x];
    __syncthreads();
    const AluUnit& un = tab.unit[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool over = false, unk = false;
    if (t < n) {
        bool hc;
        const uint64_t c = int_load(un.op + t * 8, &hc);
        unk = hc || c >= n_prog;
        uint64_t r0 = 0, r1 = 0;
        AluEnt e = {0, 0, 0};
        if (!unk) e = prog[c];
        if (e.kind) {
            const uint32_t kind = e.kind, w = e.w_imm & 0xffu;
            const bool has_imm = (e.w_imm >> 8) != 0;
            const uint64_t mask = w == 64 ? ~0ull : (1ull << w) - 1, top_bit = 1ull << (w - 1);
            bool ha = false, hb = false;
            uint64_t ra = c, rb = e.imm;            // (an op cell that is read as an operand is below n_prog: a machine word)
            if (un.a != un.op) ra = int_load(un.a + t * 8, &ha);
            if (!has_imm) {
                if (un.b == un.op) {
                    rb = c;
                } else if (un.b == un.a) {
                    rb = ra;
                    hb = ha;
                } else {
                    rb = int_load(un.b + t * 8, &hb);
                }
            }
            const uint64_t a = ra & mask;
            over = ha || a != ra;
            const bool is_shift = kind >= KZG_ALU_SLL && kind <= KZG_ALU_ROTR;
            const bool is_sdiv = kind == KZG_ALU_DIV || kind == KZG_ALU_REM;
            const bool is_udiv = kind == KZG_ALU_DIVMOD || kind == KZG_ALU_REMU;
            uint64_t b, s = 0;                      // the second operand as a number, and as a shift or a field width
            if (kind == KZG_ALU_SPLIT) {            // a shift in [0, w]
                const bool bad = hb || rb > w;
                b = s = bad ? w : rb;
                over |= bad;
            } else if (kind == KZG_ALU_SEXT) {      // a field width in [1, w]
                const bool bad = hb || rb == 0 || rb > w;
                b = s = bad ? w : rb;
                over |= bad;
            } else {
                b = rb & mask;
                over |= hb || b != rb;
            }
            const bool sa = (a & top_bit) != 0, sb = (b & top_bit) != 0;
            // ---- the division core: quotient and remainder of magnitudes or operands, or a shift amount b mod w
            uint64_t num = a, den = b, q = 0, r = 0;
            if (is_sdiv) {
                num = sa ? (0 - a) & mask : a;
                den = sb ? (0 - b) & mask : b;
            }
            if (is_shift) {
                num = b;
                den = w;
            }
            if (is_sdiv || is_udiv || (is_shift && (w & (w - 1)) != 0)) {
                const uint64_t d = den ? den : 1;
                q = num / d;
                r = num - q * d;
            } else if (is_shift) {
                r = b & (w - 1);
            }
            if (is_shift) s = r;                    // in [0, w)
            uint64_t quo = q, rem = r;
            if (is_sdiv) {
                quo = sa != sb ? (0 - q) & mask : q;
                rem = sa ? (0 - r) & mask : r;
            }
            if (b == 0) {                           // the RISC-V convention, signed and unsigned alike
                quo = mask;
                rem = a;
            }
            // ---- the add / sub / compare core
            const uint64_t sum = a + b;             // (below 2^64 when w < 64)
            const uint64_t carry = w == 64 ? (uint64_t)(sum < a) : sum >> w;
            const uint64_t dif = (a - b) & mask, ltu = a < b, lts = (a ^ top_bit) < (b ^ top_bit), equ = a == b;
            // ---- the product core
            const uint64_t lo = a * b, hi = __umul64hi(a, b);
            const uint64_t plo = lo & mask, phi = w == 64 ? hi : (lo >> w) | (hi << (64 - w));   // (a b < 2^(2 w))
            const uint64_t hsu = (phi - (sa ? b : 0)) & mask, hss = (hsu - (sb ? a : 0)) & mask;
            // ---- the shift core: s in [0, 64], at most w
            const uint64_t fm = s >= 64 ? ~0ull : (1ull << s) - 1, low = a & fm, srl = s >= 64 ? 0 : a >> s;
            const uint64_t top = s ? a >> (w - s) : 0;                       // the top s bits (w - s = 64 only at s = 0)
            const uint64_t sll = (a << (s & 63)) & mask;
            const uint64_t sra = srl | (sa ? mask & ~(mask >> (s & 63)) : 0);
            const uint64_t rotr = s ? srl | (low << ((w - s) & 63)) : a;
            const uint64_t fbit = (low >> ((s - 1) & 63)) & 1;                // SEXT: bit f - 1
            switch (kind) {
                case KZG_ALU_AND: r0 = a & b; break;
                case KZG_ALU_OR: r0 = a | b; break;
                case KZG_ALU_XOR: r0 = a ^ b; break;
                case KZG_ALU_ADD: r0 = sum & mask; r1 = carry; break;
                case KZG_ALU_SUB: r0 = dif; r1 = ltu; break;
                case KZG_ALU_MUL: r0 = plo; r1 = phi; break;
                case KZG_ALU_DIVMOD: r0 = quo; r1 = rem; break;
                case KZG_ALU_SPLIT: r0 = srl; r1 = low; break;
                case KZG_ALU_LTU: r0 = ltu; r1 = dif; break;
                case KZG_ALU_LT: r0 = lts; r1 = dif; break;
                case KZG_ALU_EQ: r0 = equ; r1 = dif; break;
                case KZG_ALU_SLL: r0 = sll; r1 = top; break;
                case KZG_ALU_SRL: r0 = srl; r1 = low; break;
                case KZG_ALU_SRA: r0 = sra; r1 = low; break;
                case KZG_ALU_ROTL: r0 = sll | top; r1 = top; break;
                case KZG_ALU_ROTR: r0 = rotr; r1 = low; break;
                case KZG_ALU_MULHU: r0 = phi; r1 = plo; break;
                case KZG_ALU_MULH: r0 = hss; r1 = plo; break;
                case KZG_ALU_MULHSU: r0 = hsu; r1 = plo; break;
                case KZG_ALU_DIV: r0 = quo; r1 = rem; break;
                case KZG_ALU_REM: r0 = rem; r1 = quo; break;
                case KZG_ALU_REMU: r0 = rem; r1 = quo; break;
                default: r0 = fbit ? low | (mask & ~fm) : low; r1 = fbit; break;   // KZG_ALU_SEXT
            }
        }
        int_store(un.out + t * 8, r0);
        if (un.count == 2) int_store(un.out + (T + t) * 8, r1);
    }
    derive_count(over, counts + blockIdx.y);
    derive_count(unk, unknown + blockIdx.y);
    expr_first(over, first + blockIdx.y);
    expr_first(unk, first_unknown + blockIdx.y);
}

void launch_alu(hipStream_t s, const AluTab& tab, uint32_t n_prog, uint32_t n_units, uint64_t T, uint64_t n, uint64_t* stats) {
    if (!n || n > T || n_prog == 0 || n_prog > ALU_MAX_PROG || n_units == 0 || n_units > ALU_MAX_UNITS || !stats) return;
    bool needs_b = false;
    for (uint32_t e = 0; e < n_prog; e++) {
        const AluEnt& en = tab.prog[e];
        if (!en.kind) continue;
        const uint32_t w = en.w_imm & 0xffu;
        if (en.kind > KZG_ALU_SEXT || w == 0 || w > 64 || (en.w_imm >> 9) != 0) return;
        needs_b |= (en.w_imm >> 8) == 0;
    }
    for (uint32_t u = 0; u < n_units; u++) {
        const AluUnit& un = tab.unit[u];
        if (!un.op || !un.a || !un.out || (needs_b && !un.b) || un.count == 0 || un.count > 2) return;
    }
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    k_fr_alu<<<dim3(nblk(n, 256), n_units), 256, 0, s>>>(tab, n_prog, T, n, st, st + n_units, st + 2 * n_units, st + 3 * n_units);
}
