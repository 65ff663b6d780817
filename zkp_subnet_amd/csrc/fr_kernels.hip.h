// Fr-side kernel launchers (fr_ntt.hip: codec + NTT; fr_poly.hip: opening): wire codec, NTT, opening evaluation + quotient.
#pragma once
#include "g1.hip.h"

// one scalar as a kernel argument: the 32 big-endian bytes, as they lie in memory
struct FrArg {
    uint32_t w[8];
};
void launch_fr_from_be(hipStream_t s, const uint8_t* be, uint32_t* out, uint64_t n, int to_mont, uint32_t* bad);
// one scalar from HOST memory, handed over as a kernel argument (no copy on the stream)
void launch_fr_from_host32(hipStream_t s, const uint8_t be32[32], uint32_t* out, int to_mont, uint32_t* bad);
void launch_fr_to_be(hipStream_t s, const uint32_t* in, uint8_t* be, uint64_t n, int from_mont);
void launch_fr_from_mont(hipStream_t s, const uint32_t* in, uint32_t* out, uint64_t n);
// typed columns (kzg_rows_commit_typed): the integer columns of one call, packed into one device buffer (each starting on a
// 16-byte boundary and padded to one), decoded into rows of T Montgomery elements by ONE launch whose argument is this table.
// Column c: `count` cells of `kind` (a KZG_COL_* integer kind) at packed + off -> out + row * T * 8; cells [count, T) take
// `fill` (canonical little-endian words); cells [0, skip) are left alone (a be32 column: skip = count, its cells are
// k_fr_from_be's and the launch writes the fill behind them only).
#define FR_TYPED_MAX_COLS 16
struct TypedCol {
    uint64_t off, count, skip;
    uint32_t kind, row;
    uint32_t fill[8];
};
struct TypedTab {
    TypedCol c[FR_TYPED_MAX_COLS];
};
static_assert(sizeof(TypedTab) + 64 <= 4096, "the column table rides as a kernel argument");
void launch_fr_from_typed(hipStream_t s, const uint8_t* packed, const TypedTab& tab, uint32_t ncols, uint32_t* out, uint64_t T);
// cells [first, first + count) of the Montgomery row `in` narrowed to `kind` (kzg_rows_read): KZG_COL_BE32 writes 32 big-endian
// bytes per cell, an integer kind its width; ovf[0] counts the cells that do not fit (written as 0), ovf[1] holds
// UINT64_MAX - the smallest such cell (0: none).  The caller zeroes ovf.
void launch_fr_narrow(hipStream_t s, const uint32_t* in, uint64_t first, uint64_t count, uint32_t kind, uint8_t* out,
                      uint64_t* ovf);
// tw: 2^(log_n-1) Montgomery-form powers of w_n (inverse: of w_n^-1), 12 words each (nine limbs + padding)
void launch_fr_twiddles(hipStream_t s, uint32_t* tw, int log_n, int inverse);
void launch_fr_inv_pow2(hipStream_t s, uint32_t* out, int log_n);
// out-of-place natural-order NTT of 2^log_n Montgomery-form elements; scale (1/n, Montgomery) applied if given
// tw: the table launch_fr_twiddles fills (n/2 twiddles, nine 29-bit limbs in a 48-byte slot each).  mid: 12 * n words of
// scratch (the vector between passes, same slot format); unused when log_n <= 8 (one pass)
void launch_fr_ntt(hipStream_t s, const uint32_t* in, uint32_t* out, int log_n, const uint32_t* tw,
                   const uint32_t* scale_or_null, uint32_t* mid);
// launch_fr_ntt is "plan, then run" (fr_ntt.hip).  A plan: the kernel form and, per pass, the stages S and the log2 of the
// tile's columns; ntt_plan is the launcher's arithmetic as a pure host function, ntt_production_plan what launch_fr_ntt
// picks (the 2^18 switch, KZG_NTT_RADIX2, KZG_NTT_TILE_LOG), ntt_plan_invalid the kernels' preconditions (null: valid),
// run_fr_ntt_plan the launches of a valid plan (arguments as launch_fr_ntt, log_n >= 1).
#define NTT_MAX_PASSES 8
struct NttPlan {
    int radix2, passes;
    int S[NTT_MAX_PASSES], logC[NTT_MAX_PASSES];
};
NttPlan ntt_plan(int log_n, bool radix2, int tile_log);
// kernel -1 / 0 / 1: the production choice / register-blocked / radix-2; tile_log 0: the production tile, 8 .. 11: that one
NttPlan ntt_plan_for(int log_n, int kernel, int tile_log);
NttPlan ntt_production_plan(int log_n);
const char* ntt_plan_invalid(int log_n, const NttPlan& pl);
void run_fr_ntt_plan(hipStream_t s, const uint32_t* in, uint32_t* out, int log_n, const uint32_t* tw,
                     const uint32_t* scale_or_null, uint32_t* mid, const NttPlan& pl);
// y = f(alpha) (Montgomery) and, if q is given, the n-1 canonical coefficients of (f - y)/(X - alpha)
// h, hnext: poly_level_words(n) words of scratch each -- ceil(n/4) * 3/2 + 64 Fr (level arrays stacked; the chunk length
// shrinks to 4 for small rows); the product and sum scans of the row-set builders size theirs the same way
// alpha_be32_host given: alpha arrives as 32 big-endian HOST bytes (a kernel argument of the first kernel), its
// Montgomery form is left at alpha_mont, *bad is raised if it is >= r; otherwise alpha_mont is read.
// y_be_or_null: also write y as 32 big-endian bytes (device pointer)
inline uint64_t poly_level_words(uint64_t n) {
    const uint64_t nchunks = (n + 3) / 4;
    return (nchunks + (nchunks >> 1) + 64) * 8;
}
void launch_poly_open(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t* alpha_mont, uint32_t* h,
                      uint32_t* hnext, uint32_t* y_mont, uint32_t* q_canon_or_null,
                      const uint8_t* alpha_be32_host = nullptr, uint32_t* bad = nullptr, uint8_t* y_be_or_null = nullptr);
// The four opening launchers are "plan, then run" (fr_poly.hip).  A plan: the level-0 chunk 2^l0, the chunk 2^lup of every
// level above it, the most values the single-workgroup scan is left with, the scan's lanes, whether the quotient is the
// LDS-staged one, and the level table these give for n coefficients: level k folds chunks of 2^l[k] of its n[k] values
// (level 0: the coefficients) into level k + 1, whose values weigh alpha^(2^sq[k + 1]) each and start at entry off[k + 1]
// of h / hnext; level K goes to the scan.  poly_plan is what the launchers pick (l0 by length, 2048, 1024 lanes for a top
// level of more than 1024 values, KZG_POLY_NO_LDS / KZG_POLY_LDS_MIN_LOG -- read nowhere else); poly_plan_levels a
// caller's choice; poly_plan_invalid the kernels' preconditions (null: valid): l0 in 2 .. 4, scan_max >= 1, at most
// POLY_MAX_LEVELS levels, 256 or 1024 lanes, the LDS quotient only with l0 = 4 on whole blocks of 1024 coefficients, and
// the stacked levels inside poly_level_words(n).  The overloads that take a plan run it unchecked.
#define POLY_MAX_LEVELS 14
struct PolyPlan {
    int l0, lup, scan_nt, lds;
    uint64_t scan_max;
    int K;
    int l[16], sq[16];
    uint64_t n[16], off[16];
};
PolyPlan poly_plan(uint64_t n);
PolyPlan poly_plan_levels(uint64_t n, int l0, uint64_t scan_max, int scan_nt, bool lds);
const char* poly_plan_invalid(const PolyPlan& pl, uint64_t n);
void launch_poly_open(hipStream_t s, const PolyPlan& pl, const uint32_t* f_mont, uint64_t n, uint32_t* alpha_mont, uint32_t* h,
                      uint32_t* hnext, uint32_t* y_mont, uint32_t* q_canon_or_null, const uint8_t* alpha_be32_host,
                      uint32_t* bad, uint8_t* y_be_or_null);
// the batched opening: y_r = f_r(alpha) for `rows` rows of n Montgomery coefficients at a stride of n elements, in the
// launches of ONE evaluation (row index in the grid).  h, hnext: rows x h_row_words words of scratch each (h_row_words >=
// 8 x the single-row size above); y_mont: rows x 8 words; y_be: rows x 32 bytes; alpha as in launch_poly_open
void launch_poly_eval_rows(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t rows, uint32_t* alpha_mont,
                           uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                           const uint8_t* alpha_be32_host, uint32_t* bad, uint8_t* y_be);
void launch_poly_eval_rows(hipStream_t s, const PolyPlan& pl, const uint32_t* f_mont, uint64_t n, uint32_t rows,
                           uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                           const uint8_t* alpha_be32_host, uint32_t* bad, uint8_t* y_be);
// out[t] = sum_j gamma^j rows[j * n + t] (Montgomery in and out), j < k <= 16; gamma as 32 big-endian HOST bytes (a kernel
// argument), *bad raised when it is >= r
void launch_fr_combine_rows(hipStream_t s, const uint32_t* rows_mont, uint64_t n, uint32_t k, const uint8_t gamma_be32_host[32],
                            uint32_t* out_mont, uint32_t* bad);
// the multi-point opening (kzg_commit_open_multi): up to POLY_MAX_POINTS points and POLY_MAX_PAIRS (row, point) pairs of
// one launch, all as kernel arguments.  pa.a[p]: point p's 32 big-endian bytes; pair y = row pa.row[y] at point pa.pt[y],
// point-major (a point's pairs are consecutive).
#define POLY_MAX_POINTS 4
#define POLY_MAX_PAIRS 64
struct PairArg {
    FrArg a[POLY_MAX_POINTS];
    uint8_t row[POLY_MAX_PAIRS], pt[POLY_MAX_PAIRS];
};
// where the opened rows live: row j's n Montgomery coefficients start at r[j] (a kernel argument beside PairArg / CombArg).
// kzg_commit_open_multi fills it with its strided rows, kzg_rows_open with rows of its committed sets, wherever they lie.
#define POLY_MAX_ROWS 16
struct RowTab {
    const uint32_t* r[POLY_MAX_ROWS];
};
// y_t = f_{row[t]}(alpha_{pt[t]}) for `npairs` pairs over rows of n Montgomery coefficients (row j at rt.r[j]), in the
// launches of ONE evaluation.  alpha_mont: POLY_MAX_POINTS x 8 words, each point's Montgomery form is left there (*bad
// raised for a point >= r); h, hnext: npairs x h_row_words words each (as launch_poly_eval_rows); y_mont: npairs x 8 words;
// y_be: npairs x 32 bytes
void launch_poly_eval_pairs(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t npairs, const PairArg& pa,
                            uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                            uint32_t* bad, uint8_t* y_be);
void launch_poly_eval_pairs(hipStream_t s, const PolyPlan& pl, const RowTab& rt, uint64_t n, uint32_t npairs, const PairArg& pa,
                            uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                            uint32_t* bad, uint8_t* y_be);
// m openings side by side: f_p = f_mont + p * n elements at the point alpha_mont + 8 p (Montgomery, already in memory):
// y_p at y_mont + 8 p and the n-1 canonical quotient coefficients (slot n - 1 zero) at q_canon + p * n elements
// (y_be given: y_p also as 32 big-endian bytes at y_be + 32 p)
void launch_poly_open_points(hipStream_t s, const uint32_t* f_mont, uint64_t n, uint32_t m, const uint32_t* alpha_mont,
                             uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont, uint32_t* q_canon,
                             uint8_t* y_be = nullptr, const uint8_t* pts = nullptr, bool q_mont = false);
void launch_poly_open_points(hipStream_t s, const PolyPlan& pl, const uint32_t* f_mont, uint64_t n, uint32_t m,
                             const uint32_t* alpha_mont, uint32_t* h, uint32_t* hnext, uint64_t h_row_words, uint32_t* y_mont,
                             uint32_t* q_canon, uint8_t* y_be, const uint8_t* pts, bool q_mont);
// out[t] = (accumulate ? out[t] : 0) + sum_{g < cnt} rt.r[g][t] over n elements (Montgomery in and out, reduced below r):
// the sum of the groups' final quotients of kzg_rows_commit_shplonk
void launch_fr_sum_rows(hipStream_t s, const RowTab& rt, uint32_t cnt, uint64_t n, bool accumulate, uint32_t* out_mont);
// h_p[t] = sum gamma_p^j rt.r[j][t] over the rows j of mask[p] (Montgomery in and out) into out + p * n elements, for
// p < m in one launch; g[p]: gamma_p's 32 big-endian bytes, *bad raised when one is >= r
struct CombArg {
    FrArg g[POLY_MAX_POINTS];
    uint32_t mask[POLY_MAX_POINTS];
};
void launch_fr_combine_points(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t m, const CombArg& ca,
                              uint32_t* out_mont, uint32_t* bad);
// the caller-weighted combinations of kzg_rows_open_lincomb, p < m in one launch: h_p[t] = sum_j lambda_{p,j} rt.r[j][t]
// (Montgomery in and out) into out + p * n elements.  coeffs_be32: m x k canonical scalars, point-major; masks[p] bit j set
// exactly when lambda_{p,j} != 0 (the rows the kernel reads).  Point p (32 big-endian bytes at points_be32 + 32 p) is
// converted by the launch and left at alpha_mont + 8 p for the openings behind it.  *bad raised for a coefficient or a
// point >= r.  The launcher packs all of it into ONE kernel argument (2.4 KB at m = 4, k = 16).
// alpha_mont == null (the group combinations of kzg_rows_commit_shplonk, "point" read as "group of rows with one point
// set"): no point is converted and points_be32 is not read.
void launch_fr_lincomb_points(hipStream_t s, const RowTab& rt, uint64_t n, uint32_t m, uint32_t k, const uint8_t* coeffs_be32,
                              const uint32_t* masks, const uint8_t* points_be32, uint32_t* out_mont, uint32_t* alpha_mont,
                              uint32_t* bad);
// *flag |= 1 when a[0, n_words) and b[0, n_words) differ (n_words a multiple of 4): verification of a row-cache hit
void launch_words_differ(hipStream_t s, const uint32_t* a, const uint32_t* b, uint64_t n_words, uint32_t* flag);
// ---- the permutation grand product (fr_prod.hip; kzg_rows_commit_grand_product)
// one wire / sigma pair folded into the running vectors: N[t] (*)= ea[t] + beta s w^t + gamma, D[t] (*)= ea[t] + beta es[t] +
// gamma (first: written instead of multiplied).  ea, es: the pair's n evaluations (Montgomery, natural order); tw: the forward
// table of launch_fr_twiddles for n (unused when n == 1); beta, gamma, s as 32 big-endian HOST bytes, *bad raised when >= r
void launch_gp_factors(hipStream_t s, const uint32_t* ea, const uint32_t* es, uint32_t* N, uint32_t* D, uint64_t n,
                       const uint32_t* tw, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                       const uint8_t shift_be32[32], bool first, uint32_t* bad);
// kzg_rows_commit_shuffle: one side of one group folded into its running vector: with v = acc theta + e (acc given) or e,
// V[t] (*)= gamma + v, or 1 + sel[t] (gamma + v - 1) when sel is given (first: written instead of multiplied).  e, acc, sel: n
// canonical Montgomery elements each; theta, gamma as 32 big-endian HOST bytes, *bad raised when >= r
void launch_sh_factor(hipStream_t s, const uint32_t* e, const uint32_t* acc_or_null, uint32_t* V, const uint32_t* sel_or_null,
                      uint64_t n, const uint8_t theta_be32[32], const uint8_t gamma_be32[32], bool first, uint32_t* bad);
// N[t] <- z(w^t) = (prod_{u<t} N_u) (prod_{u>=t} D_u) / prod_u D_u (D is consumed); scrN, scrD: (n + 3) / 4 * 3 / 2 + 64
// elements of scratch each.  closing_be (device): prod N / prod D, 32 bytes big-endian; *zero_flag (device): 1 when
// prod D == 0 (z undefined, N then holds zeros), else 0
// start_be32 (kzg_rows_commit_grand_product_chain; null: 1): every z(w^t) and the closing value are multiplied by it -- 32
// big-endian HOST bytes, canonical and nonzero (the caller's check), folded into the top level's <= 2048 prefix values
void launch_gp_scan(hipStream_t s, uint32_t* N, uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                    uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32 = nullptr);
// the scan without its last level (N and D only read; they may be one vector): scrN[g] / scrD[g] <- the exclusive prefix
// product of N in front of level-0 chunk g / the exclusive suffix product of D behind it times 1 / prod D; closing_be and
// zero_flag as above.  Returns log2 of the level-0 chunk length.  n > 0
int launch_gp_scan_upper(hipStream_t s, const uint32_t* N, const uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                         uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32 = nullptr);
// test hook: out[j] = in[j]^-1 (32 big-endian bytes each, canonical; 0 for in[j] == 0) or, with want_flag, the inversion's
// zero flag (0 / 1) in the same format
void launch_fr_inv_test(hipStream_t s, const uint8_t* in_be, uint8_t* out_be, uint64_t n, int want_flag);
// ---- the PLONK quotient (fr_quot.hip; kzg_rows_commit_quotient): T = 2^log_t, E = 2^ext_log, N = E T, coset g H_N with g = 7
#define QUOT_MAX_TERMS 16
#define QUOT_MAX_FACTORS 9   // E + 1 at E = 8
#define QUOT_MAX_WIRES 8     // k <= E
// the constraints, rows named by index into the table of extended vectors; scalars as 32 big-endian HOST bytes each
struct QuotPlan {
    uint32_t ext_log, n_terms, k, z_row;
    uint8_t term_len[QUOT_MAX_TERMS], term_row[QUOT_MAX_TERMS][QUOT_MAX_FACTORS], wire[QUOT_MAX_WIRES], sigma[QUOT_MAX_WIRES];
    const uint8_t *term_coeffs_be32, *shifts_be32, *beta_be32, *gamma_be32, *alpha_be32;   // (the last four unused when k == 0)
    // kzg_rows_commit_quotient_ext.  ext == 0: nothing below is read and the plain call's kernel runs.  Gate factor f of term
    // u is row term_row[u][f] at w^rot X, rot = term_rot[u][f] in [0, T); n_lookups > 0 adds alpha^3 LK1 + alpha^4 LK2 over
    // the n_lookups * width rows in_row (lookup-major), the width rows tab_row, m = mult_row and S = sum_row, with theta_be32,
    // lbeta_be32 and alpha_be32 (then read when k == 0 too)
    uint32_t ext, n_lookups, width, mult_row, sum_row;
    uint32_t term_rot[QUOT_MAX_TERMS][QUOT_MAX_FACTORS];
    uint8_t in_row[POLY_MAX_ROWS], tab_row[POLY_MAX_ROWS];
    const uint8_t *theta_be32, *lbeta_be32;
    // kzg_rows_commit_quotient_zk.  active != 0 (then ext != 0 too): P1 and LK1 are multiplied by row active_row, the caller's
    // column A that is 1 on the usable rows and 0 elsewhere, and the third instantiation of the kernel runs
    uint32_t active, active_row;
    // kzg_rows_quotient_part with a link.  link != 0 (then ext != 0 and k > 0): P2 = (z - f_prev(w^rot X)) L_0 with f_prev = row
    // link_row and rot = link_rot in [0, T), and a linked instantiation of the kernel runs
    uint32_t link, link_row, link_rot;
    // kzg_rows_commit_quotient_sel / kzg_rows_quotient_part_sel.  sel != 0 (then ext != 0 and n_lookups > 0): lookup l's fraction in
    // LK1 has the numerator row sel_row[l] (0xff: the constant 1), and a SEL kernel runs.  sel == 0: sel_row is not read
    uint32_t sel;
    uint8_t sel_row[POLY_MAX_ROWS];
};
// the constants record of one (T, E), in 8-word elements: 1 / Z_H on the coset, 1 / T, g and the power tables of g and 1 / g
uint64_t quot_consts_elems(int log_t, int ext_log);
// tw_n: the forward table of launch_fr_twiddles for N (also below)
void launch_quot_consts(hipStream_t s, uint32_t* qc, int log_t, int ext_log, const uint32_t* tw_n);
// ext[i] = g^i f[i] for i < T, 0 for T <= i < N (f: T Montgomery coefficients; null: the coefficients of L_0, all 1 / T)
void launch_quot_extend(hipStream_t s, const uint32_t* f_or_null, uint32_t* ext, int log_t, int ext_log, const uint32_t* qc);
// out[i] = (Gate + alpha [A] P1 + alpha^2 P2 + alpha^3 [A] LK1 + alpha^4 LK2)(x_i) / Z_H(x_i) over the rows' N coset evaluations
// ext_rows.r[.] and L_0's l0 (unused when k == 0 and n_lookups == 0); out must not alias a row (z and S are read at i + E, a
// rotated factor at i + rot E).  *bad raised for a scalar >= r
void launch_quot_points(hipStream_t s, const RowTab& ext_rows, const uint32_t* l0, uint32_t* out, int log_t, const QuotPlan& qp,
                        const uint32_t* tw_n, const uint32_t* qc, uint32_t* bad);
// in: the N coefficients of t(g X) (inverse transform, 1 / N applied).  dst[i] = g^-i in[i] for i < n_pieces T (the pieces,
// consecutive); *tail_flag |= 1 when some in[i], i >= n_pieces T, is not zero
void launch_quot_pieces(hipStream_t s, const uint32_t* in, uint32_t* dst, int log_t, int ext_log, uint32_t n_pieces,
                        const uint32_t* qc, uint32_t* tail_flag);
// acc[i] = scale v[i] (first) or acc[i] + scale v[i] over n canonical Montgomery elements, canonical on store; scale: 32
// big-endian HOST bytes < r (the caller's check), null: 1.  The add of kzg_rows_quotient_part
void launch_quot_accumulate(hipStream_t s, uint32_t* acc, const uint32_t* v, uint64_t n, const uint8_t* scale_be32_or_null,
                            bool first);
// ---- the lookup (logUp) running sum (fr_lookup.hip; kzg_rows_commit_lookup_sum)
// one transformed column e (n evaluations, Montgomery) folded in: v = acc theta + e (has_acc) or e, then by mode
//   0: acc <- v    1: Q <- beta + v, P <- -P (P holds m's evaluations)    2: (P, Q) <- (P d + Q, Q d), d = beta + v
// theta, beta as 32 big-endian HOST bytes, *bad raised when >= r
void launch_lk_step(hipStream_t s, const uint32_t* e, uint32_t* acc, uint32_t* P, uint32_t* Q, uint64_t n, int mode,
                    bool has_acc, const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint32_t* bad);
// mode 2 with a numerator (kzg_rows_commit_lookup_sum_sel): (P, Q) <- (P d + q Q, Q d), q = sel[t], n canonical Montgomery
// elements (the lookup's selector row in evaluation form)
void launch_lk_step_sel(hipStream_t s, const uint32_t* e, uint32_t* acc, uint32_t* P, uint32_t* Q, const uint32_t* sel,
                        uint64_t n, bool has_acc, const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint32_t* bad);
// The batched inversion: out[t] <- 1 / Q[t], or P[t] / Q[t] when P is given, for n Montgomery elements with ONE fr9_inv:
// 1 / Q_t = (prod_{u<t} Q_u) (prod_{u>t} Q_u) / prod_u Q_u.  Q is only read; W: n elements of workspace; out may be W or P.
// scrN, scrD: (n + 3) / 4 * 3 / 2 + 64 elements of scratch each; scratch32 (device): 32 bytes that are overwritten;
// *zero_flag (device): 1 when some Q[t] == 0 (out then holds zeros), else 0
void launch_fr_batch_inv(hipStream_t s, const uint32_t* Q, uint32_t* W, const uint32_t* P_or_null, uint32_t* out, uint64_t n,
                         uint32_t* scrN, uint32_t* scrD, uint8_t* scratch32, uint32_t* zero_flag);
// v[t] <- sum_{u<t} v[u] in place (n Montgomery elements, canonical); scr: (n + 3) / 4 * 3 / 2 + 64 elements; closing_be
// (device): sum_u v[u], 32 bytes big-endian
void launch_lk_sum_scan(hipStream_t s, uint32_t* v, uint64_t n, uint32_t* scr, uint8_t* closing_be);
// ---- the hash join of the lookup multiplicities (fr_join.hip; kzg_rows_commit_multiplicities).  tab / in: w columns of T
// canonical Montgomery elements each, column c at + c * T * 8 words; slots: cap u32 (cap a power of two >= 2 T, all
// 0xffffffff before the build); *overrun (device) raised when a probe walk reaches its bound of cap steps
// slot[..] <- the smallest row index of every distinct table tuple
void launch_join_build(hipStream_t s, const uint32_t* tab, uint64_t T, uint32_t w, uint32_t* slots, uint32_t cap,
                       uint32_t* overrun);
// one lookup's T cells: cnt[first(tuple)] += 1 for a cell whose tuple is a table row, *missing += 1 otherwise
void launch_join_probe(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint32_t w, const uint32_t* slots,
                       uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun);
// out[t] <- cnt[t] as a canonical Montgomery element
void launch_join_counts(hipStream_t s, const uint32_t* cnt, uint32_t* out, uint64_t T);
// the same join over the first `rows` rows only (kzg_rows_commit_multiplicities_zk): the columns still lie T elements apart,
// table rows and cells at or above `rows` are neither built nor probed nor counted as missing
void launch_join_build_rows(hipStream_t s, const uint32_t* tab, uint64_t T, uint64_t rows, uint32_t w, uint32_t* slots,
                            uint32_t cap, uint32_t* overrun);
void launch_join_probe_rows(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint64_t rows, uint32_t w,
                            const uint32_t* slots, uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun);
// one lookup's first `rows` cells (rows = T: all of them) under a selector (kzg_rows_commit_multiplicities_sel): sel holds T
// canonical Montgomery elements, a cell whose sel[t] is zero is neither probed nor counted as missing
void launch_join_probe_sel(hipStream_t s, const uint32_t* tab, const uint32_t* in, const uint32_t* sel, uint64_t T, uint64_t rows,
                           uint32_t w, const uint32_t* slots, uint32_t cap, uint32_t* cnt, uint64_t* missing, uint32_t* overrun);
// test hook (kzg_test_join): home[t] <- the slot at which the walk of tuple t < n <= T of cols starts, hash & (cap - 1)
void launch_join_home(hipStream_t s, const uint32_t* cols, uint64_t T, uint32_t w, uint64_t n, uint32_t cap, uint32_t* home);
// ---- the fetch of kzg_rows_commit_fetch (fr_join.hip).  tab: n_keys + n_pay columns of T canonical Montgomery elements, the
// first n_keys of them the key that launch_join_build(_rows) was called with (w = n_keys, the same `rows`); in: the n_keys
// columns of one read; out: index + n_pay vectors of T, of which cells [0, rows) are written.  Cell t takes the payload of the
// smallest table row below `rows` whose key equals the cell's (with index: that row number first, as a canonical Montgomery
// element), or zeros; *missing += the cells without such a row, *first <- min(*first, the smallest such cell).  out must not
// overlap tab or in.  rows <= T <= 2^27
void launch_join_fetch(hipStream_t s, const uint32_t* tab, const uint32_t* in, uint64_t T, uint64_t rows, uint32_t n_keys,
                       uint32_t n_pay, bool index, const uint32_t* slots, uint32_t cap, uint32_t* out, uint64_t* missing,
                       uint64_t* first, uint32_t* overrun);
// the fetch by row index: cell t < rows of the n_pay vectors of out takes tab[p T + q], q the canonical integer of addr[t], or
// zeros where q >= rows (all 255 bits are compared); the counts as above.  tab: n_pay columns, all payload
void launch_fetch_index(hipStream_t s, const uint32_t* tab, const uint32_t* addr, uint64_t T, uint64_t rows, uint32_t n_pay,
                        uint32_t* out, uint64_t* missing, uint64_t* first);
// ---- the stable sort of kzg_rows_commit_sorted (fr_sort.hip).  ev: the columns as evaluation vectors of T canonical Montgomery
// elements, column c at + c * T * 8 words; rows [0, n) are sorted by the canonical integers of columns 0 .. n_keys - 1 (column 0
// most significant), ties by ascending row.  keys: n_keys vectors of T elements; ws: fr_sort_ws_words(n, n_keys) words
uint64_t fr_sort_ws_words(uint64_t n, uint32_t n_keys);
uint32_t fr_sort_tile();   // positions per workgroup of the per-pass kernels
// the keys' canonical integers into `keys` and the digit histograms of all 32 n_keys passes; returns the DEVICE address of the
// passes' skip words (32 n_keys x u32, 1: one bin holds all n rows, the pass moves nothing)
const uint32_t* launch_sort_front(hipStream_t s, const uint32_t* ev, uint64_t T, uint64_t n, uint32_t n_keys, uint32_t* keys,
                                  uint32_t* ws);
// the passes whose skip word (HOST copy) is 0; returns the final permutation (n x u32 inside ws; row perm[t] of the source is
// row t of the result), or null when no pass ran: the identity
const uint32_t* launch_sort_passes(hipStream_t s, const uint32_t* keys, uint64_t T, uint64_t n, uint32_t n_keys,
                                   const uint32_t* skip_host, uint32_t* ws);
// out[t] = col[perm[t]] for t < n (perm null: the identity); col and out must not overlap
void launch_sort_gather(hipStream_t s, const uint32_t* col, const uint32_t* perm, uint32_t* out, uint64_t n);
// v[usable + j] <- tail[j], j < n - usable <= BLIND_MAX_ROWS (no closing row, unlike launch_blind_tail); tail_be32: canonical
// scalars as 32 big-endian HOST bytes each (a kernel argument), *bad raised when one is >= r
void launch_sort_tail(hipStream_t s, uint32_t* v, uint64_t n, uint64_t usable, const uint8_t* tail_be32, uint32_t* bad);
// ---- the sigma columns of kzg_rows_commit_sigma and the check of kzg_rows_check_copies (fr_sigma.hip).  The k <= SIGMA_MAX_COLS
// label columns are sorted as ONE vector of N = k n <= 2^27 cells in flat-index order (cell c n + t: column c, row t < n <= T)
// by launch_sort_front / launch_sort_passes with n_keys = 1: keys holds the cells' canonical integers, perm the sorted order
// (null: the identity).  Cells with equal keys are one class; a cell whose key is free_be32 (null: none) stands alone.
#define SIGMA_MAX_COLS POLY_MAX_ROWS
// sig[c T + t] <- shift[c'] w_T^t' (canonical Montgomery) for every cell (c, t), t < n, where (c', t') is the next larger cell of
// its class, or the smallest one behind the largest; stats[0] += the classes, stats[1] += the cells that map to themselves.
// tw: the forward twiddle table of T (launch_fr_twiddles; not read at T = 1); shifts_be32: k scalars as 32 big-endian HOST
// bytes each, free_be32 likewise (kernel arguments), *bad raised when one is >= r.  sig: k vectors of T elements
void launch_sigma_link(hipStream_t s, const uint32_t* keys, const uint32_t* perm, uint64_t N, uint64_t n, uint64_t T, uint32_t k,
                       const uint32_t* tw, const uint8_t* shifts_be32, const uint8_t* free_be32, uint32_t* sig, uint64_t* stats,
                       uint32_t* bad);
// sig[c T + t] <- shift[c] w_T^t for n <= t < T: the rows that take no part
void launch_sigma_identity(hipStream_t s, uint64_t n, uint64_t T, uint32_t k, const uint32_t* tw, const uint8_t* shifts_be32,
                           uint32_t* sig, uint32_t* bad);
// out[0] += the non-free cells whose value in wires.r[c][t] (canonical Montgomery, T elements per column) differs from that of
// their class's smallest cell, out[1] <- min(out[1], the smallest such flat index c T + t)
void launch_copy_check(hipStream_t s, const uint32_t* keys, const uint32_t* perm, uint64_t N, uint64_t n, uint64_t T, uint32_t k,
                       const RowTab& wires, const uint8_t* free_be32, uint64_t* out);
// ---- the helper columns of kzg_rows_commit_derived (fr_derive.hip).  A source is an evaluation vector of T canonical Montgomery
// elements of which rows [0, n) are read; counts are u64 words in device memory that the launches add to
// the words of one op's zero mask (1 bit per cell, 32 cells per u32 word)
uint32_t inv0_mask_words(uint64_t T);
// the n_inv <= POLY_MAX_ROWS inv0 ops side by side: Q[j T + t] <- src.r[j][t], or Montgomery 1 where that is zero or t >= n (no
// zero is left for launch_fr_batch_inv); mask[j inv0_mask_words(T) ..] <- the zero cells of op j; counts[slot[j]] += their number
void launch_inv0_prepare(hipStream_t s, const RowTab& src, const uint32_t* slot, uint32_t n_inv, uint32_t* Q, uint32_t* mask,
                         uint64_t T, uint64_t n, uint64_t* counts);
// one op behind the inversion: inv[t] <- 0 under the op's mask; bit (null: none) <- Montgomery 1 under the mask, 0 elsewhere
void launch_inv0_finish(hipStream_t s, uint32_t* inv, const uint32_t* mask, uint64_t T, uint32_t* bit_or_null);
// out[l T + t] <- limb l of src[t]'s canonical integer x, (x >> (bits l)) & (2^bits - 1), as a canonical Montgomery element, for
// l < count and t < n (1 <= bits <= 32, bits count <= 256); *over += the cells with x >= 2^(bits count).  out: count vectors of T
void launch_limbs(hipStream_t s, const uint32_t* src, uint32_t* out, uint64_t T, uint64_t n, uint32_t bits, uint32_t count,
                  uint64_t* over);
// the workgroup's count of flagged lanes added to *total: one ballot and one LDS add per wave, one global add per workgroup.
// Called by every lane of the workgroup (uniform control flow).  Shared by the kernels of fr_derive.hip and fr_expr.hip
KZG_DEV void derive_count(bool flagged, unsigned long long* __restrict__ total) {
    __shared__ uint32_t wg_cnt;
    if (threadIdx.x == 0) wg_cnt = 0;
    __syncthreads();
    const unsigned long long b = __ballot(flagged);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&wg_cnt, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && wg_cnt) atomicAdd(total, (unsigned long long)wg_cnt);
}
// the workgroup's smallest flagged cell folded into *first: the lowest set bit of each wave's ballot, one LDS minimum per wave,
// one global minimum per workgroup.  Called by every lane of the workgroup (uniform control flow); lane v stands for cell
// blockIdx.x * blockDim.x + v.  Shared by the kernels of fr_expr.hip and fr_int.hip
KZG_DEV void expr_first(bool flagged, unsigned long long* __restrict__ first) {
    __shared__ uint32_t wg_first;
    if (threadIdx.x == 0) wg_first = 0xffffffffu;
    __syncthreads();
    const unsigned long long b = __ballot(flagged);
    if ((threadIdx.x & 63u) == 0 && b) atomicMin(&wg_first, threadIdx.x + (uint32_t)__ffsll(b) - 1u);
    __syncthreads();
    if (threadIdx.x == 0 && wg_first != 0xffffffffu)
        atomicMin(first, (unsigned long long)blockIdx.x * blockDim.x + wg_first);
}
// ---- the integer ALU columns of kzg_rows_commit_int (fr_int.hip): every output cell a function of the canonical integers of one
// or two source cells, reduced to their low w bits.  An op reads a[t] and b[t] (b null: the immediate imm) for t < n and writes
// `count` vectors of T elements at out (row 0, then row 1 at out + 8 T words), canonical Montgomery.  kind: a KZG_INT_* kind
#define INT_MAX_OPS POLY_MAX_ROWS
struct IntOp {
    const uint32_t *a, *b;
    uint64_t imm;
    uint32_t* out;
    uint32_t kind, w, count, pad;
};
struct IntTab {
    IntOp op[INT_MAX_OPS];
};
static_assert(sizeof(IntTab) + 64 <= 4096, "the op table rides as a kernel argument");
// ONE launch for the n_ops <= INT_MAX_OPS ops of tab; counts[o] += the cells t < n of op o with an operand at or above 2^w
// (a SPLIT's shift cell: above w), first[o] <- min(first[o], the smallest such t).  a and b are only read and may be one
// vector; out must not overlap a source.  1 <= w <= 64, an immediate below 2^w (SPLIT: at most w): the caller's checks
void launch_int(hipStream_t s, const IntTab& tab, uint32_t n_ops, uint64_t T, uint64_t n, uint64_t* counts, uint64_t* first);
// ---- the ALU column of kzg_rows_commit_alu (fr_alu.hip): the kind of every CELL comes from an op-code column.  Cell t < n of
// unit u reads c = op[t]; c >= n_prog (or no machine word at all): unknown, the outputs are 0; prog[c].kind == 0: idle, the
// outputs are 0; else the kind, the width and the optional immediate of prog[c] act on a[t] and b[t] as a KZG_ALU_* kind says.
// A unit writes `count` vectors of T elements at out (row 0, then row 1 at out + 8 T words), canonical Montgomery
#define ALU_MAX_PROG 64
#define ALU_MAX_UNITS 8
struct AluEnt {   // 16 B: one ds_read_b128 per lane
    uint64_t imm;
    uint32_t kind, w_imm;   // kind: 0 idle, or KZG_ALU_*; w_imm: the width in the low byte, bit 8 set: the second operand is imm
};
struct AluUnit {
    const uint32_t *op, *a, *b;   // b null: every entry of the program has an immediate
    uint32_t* out;
    uint32_t count, pad;
};
struct AluTab {
    AluEnt prog[ALU_MAX_PROG];
    AluUnit unit[ALU_MAX_UNITS];
};
static_assert(sizeof(AluEnt) == 16 && sizeof(AluTab) + 64 <= 4096, "the program and the units ride as a kernel argument");
// ONE launch for the n_units <= ALU_MAX_UNITS units of tab over one program of n_prog <= ALU_MAX_PROG entries.  stats: four
// runs of n_units words: [u] += the cells with an operand out of range, [n_units + u] += the cells with an unknown op-code,
// [2 n_units + u] <- min(., the smallest out-of-range row), [3 n_units + u] <- min(., the smallest unknown row).  Sources are
// only read and may coincide; out must not overlap a source.  Widths, immediates and kinds: the caller's checks
void launch_alu(hipStream_t s, const AluTab& tab, uint32_t n_prog, uint32_t n_units, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the multi-limb integer columns of kzg_rows_commit_wide (fr_wide.hip).  A wide operand is `limbs` vectors of T elements
// among the source vectors at src: limb l of operand w is vector slot[w][l] (src + slot T 8 words).  An op reads its operands
// at rows t < n and writes `count` vectors of T elements at out, side by side, canonical Montgomery.  kind: a KZG_WIDE_* kind;
// flags: KZG_WIDE_NEG_C and the three bits below; imm: operand b where it is no row (absent: 1), m: the modulus, both as 16
// little-endian 32-bit words
#define WIDE_MAX_OPS 8
#define WIDE_MAX_LIMBS 8
#define WIDE_A 0
#define WIDE_B 1
#define WIDE_C 2
#define WIDE_Q 3
#define WIDE_R 4
#define WIDE_F_ROW_B 0x100u   // operand b is a run of rows
#define WIDE_F_ROW_C 0x200u   // there is an operand c
#define WIDE_F_B_IS_A 0x400u  // every limb of b is the vector of that limb of a
struct WideOp {
    uint32_t* out;
    uint32_t kind, bits, limbs, count, flags, pad;
    uint8_t slot[5][WIDE_MAX_LIMBS];
    uint32_t imm[16], m[16];
};
struct WideTab {
    WideOp op[WIDE_MAX_OPS];
    const uint32_t* src;
};
static_assert(sizeof(WideTab) + 64 <= 4096 && POLY_MAX_ROWS <= 256, "the op table rides as a kernel argument; slots ride in bytes");
// ONE launch for the n_ops <= WIDE_MAX_OPS ops of tab, instantiated on the widest b limbs of the call.  stats: four runs of
// n_ops words: [o] += the rows t < n of op o with a limb at or above 2^b (or c > m under KZG_WIDE_NEG_C), [n_ops + o] += the rows
// whose quotient does not fit W bits (mulmod) or whose limb identity is inexact (carry), [2 n_ops + o] <- min(., the smallest
// row of the first kind), [3 n_ops + o] <- min(., of the second).  Sources are only read and may coincide; out must not overlap
// a source.  1 <= b <= 64 (carry: 56), 1 <= L <= 8, b L <= 512, immediates below 2^(b L), m != 0: the caller's checks
void launch_wide(hipStream_t s, const WideTab& tab, uint32_t n_ops, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the Poseidon permutation columns of kzg_rows_commit_poseidon (fr_poseidon.hip).  The state of a unit is t elements, element
// j read from source vector slot[j] (src + slot T 8 words) or, at POS_IMM, the unit's immediate j.  A ROW unit runs one
// permutation per row t' < n and writes state element i to vector col[i] of out (POS_NO_COL: not written); with out null it is a
// check and compares that element with source vector exp[col[i]] instead.  A ROUNDS unit runs one permutation per block of
// `period` rows and writes the state before every round and behind the last into the t vectors at out, which the caller has
// zeroed.  cst: the constants as 8 little-endian 32-bit words of a canonical integer each: t R round constants, t t matrix
// entries, then t immediates per unit
#define POS_MAX_T 8
#define POS_MAX_UNITS 8
#define POS_MAX_ROUNDS 144
#define POS_ROW 1
#define POS_ROUNDS 2
#define POS_IMM 0xffu
#define POS_NO_COL 0xffu
struct PosUnit {
    uint32_t* out;
    uint32_t mode, period;
    uint8_t slot[POS_MAX_T], col[POS_MAX_T], exp[POS_MAX_T];
};
struct PosTab {
    PosUnit u[POS_MAX_UNITS];
    const uint32_t *src, *cst;
    uint32_t t, full, partial, n_units;
};
static_assert(sizeof(PosTab) + 64 <= 4096 && POLY_MAX_ROWS < POS_IMM, "the unit table rides as a kernel argument; slots ride in bytes");
// the words of cst that a call of n_units units needs, and ONE launch for all of them, instantiated on t.  stats: two runs of
// n_units words: [u] += the rows of check u with a cell that differs, [n_units + u] <- min(., the smallest such row).  Sources are
// only read and may coincide; out must not overlap a source.  2 <= t <= 8, full even, full + partial <= POS_MAX_ROUNDS, period >=
// full + partial + 1, canonical constants: the caller's checks
uint32_t poseidon_cst_words(uint32_t t, uint32_t rounds, uint32_t n_units);
void launch_poseidon(hipStream_t s, const PosTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the Poseidon2 permutation columns of kzg_rows_commit_poseidon2 (fr_poseidon2.hip).  The table is PosTab and the units are
// PosUnit exactly as launch_poseidon reads them, with two differences: a ROUNDS unit writes the input at its block's first row,
// E(input) at the next and the state behind round rho at row 2 + rho (period >= full + partial + 2); cst holds t x full
// full-round constants (round-major over both halves), `partial` partial-round constants, t diagonal entries, then t
// immediates per unit.  t in {2, 3, 4, 8}; stats as for launch_poseidon
uint32_t poseidon2_cst_words(uint32_t t, uint32_t full, uint32_t partial, uint32_t n_units);
void launch_poseidon2(hipStream_t s, const PosTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the Poseidon sponge and Merkle-path chains of kzg_rows_commit_poseidon_chain (fr_poseidon_chain.hip).  t, full, partial and
// cst are PosTab's (t immediates per unit).  A unit walks the blocks of `period` rows, b < floor(n / period); block b starts a
// segment where b = 0, `start` is PCH_NONE or the cell of source vector `start` at the block's first row is not zero, and
// continues the block before otherwise.  SPONGE: slot[j] is the source vector of state element j or POS_IMM; a continuing block
// adds its cells to the output before it and leaves an immediate's element as it is.  PATH (t >= 3): slot[0] is the cap (element
// 0), slot[1] the leaf, both a vector or POS_IMM, slot[2 + k], k < t - 2, the vector of sibling k; `pos` the vector of the child
// position; the child at that position is the leaf (a starting block) or element `digest` of the output before.  layout
// PCH_TRACE: the state before every round and behind the last into the t vectors at out; PCH_FLAT: at the block's first row
// only, arranged state element j into vector col[j] of out and output element j into vector col[POS_MAX_T + j] (PCH_NONE: not
// written); out was zeroed by the caller.  out null, layout 0, exp a source vector: a check: element `digest` of the output of a
// segment's LAST block is compared with the cell of vector exp at that block's first row
#define PCH_MAX_UNITS 4
#define PCH_SPONGE 1
#define PCH_PATH 2
#define PCH_TRACE 1
#define PCH_FLAT 2
#define PCH_NONE 0xffu
struct PchUnit {
    uint32_t* out;
    uint32_t mode, layout, period, pad;
    uint8_t slot[POS_MAX_T], col[2 * POS_MAX_T];
    uint8_t start, pos, digest, exp;
};
struct PchTab {
    PchUnit u[PCH_MAX_UNITS];
    const uint32_t *src, *cst;
    uint32_t t, full, partial, n_units;
};
static_assert(sizeof(PchTab) + 64 <= 4096 && PCH_NONE == POS_IMM, "the unit table rides as a kernel argument; one escape value");
// ONE launch for all units, instantiated on t.  stats: five runs of n_units words: [u] += the segments started, [n_units + u] +=
// the blocks whose pos cell is at or above t - 1 (read as position 0), [2 n_units + u] += the segments of a check whose digest
// differs, [3 n_units + u] <- min(., the smallest row of the second kind), [4 n_units + u] <- min(., of the third).  Sources are
// only read and may coincide; out must not overlap a source.  Returns without a launch on a table that the caller's checks
// should have refused
void launch_poseidon_chain(hipStream_t s, const PchTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the SHA-256 compression columns of kzg_rows_commit_sha256 (fr_sha256.hip).  Every value is a 32-bit word: the low 32 bits
// of a source cell's canonical integer in, int_store's cell out.  Source vector d lies at src + d T 8 words.  A ROW unit runs one
// compression per row t' < n: slot j < 8 is word j of the chaining value, slot 8 + j word j of the block; slot[j] is an index
// into the unit's list ld of n_ld DISTINCT source vectors (each cell is loaded once) or SHA_IMM: then the word is imm[j].  It
// writes word col[c] of the new chaining value to vector c < n_out of out; with out null it is a check and compares that word
// with the cell of source vector exp[c].  A ROUNDS unit walks the blocks of `period` rows: ld[0] is the message vector, ld[1]
// the start vector (SHA_IMM: every block starts a message), imm[0 .. 7] the chaining value a message starts from; it writes
// column id col[c] (SHA_COL_*) to vector c < n_out of out, which the caller has zeroed
#define SHA_MAX_UNITS 4
#define SHA_ROW 1
#define SHA_ROUNDS 2
#define SHA_IMM 0xffu
#define SHA_MIN_PERIOD 72
#define SHA_N_COLS 12
#define SHA_LANE_WORDS 36   // LDS words per lane: ROUNDS: 16 of the window, 8 of H, 12 of a row; ROW: up to 16 loaded words
enum { SHA_COL_W, SHA_COL_A, SHA_COL_E, SHA_COL_CW, SHA_COL_CA, SHA_COL_CE, SHA_COL_SIG0, SHA_COL_SIG1, SHA_COL_SUM0, SHA_COL_MAJ,
       SHA_COL_SUM1, SHA_COL_CH };
struct ShaUnit {
    uint32_t* out;
    uint32_t mode, period, n_out, n_ld;
    uint32_t imm[24];
    uint8_t slot[24], ld[24], col[SHA_N_COLS], exp[8];
};
struct ShaTab {
    ShaUnit u[SHA_MAX_UNITS];
    const uint32_t* src;
    uint32_t n_units;
};
static_assert(sizeof(ShaTab) + 64 <= 4096 && POLY_MAX_ROWS < SHA_IMM && POLY_MAX_ROWS <= SHA_LANE_WORDS,
              "the unit table rides as a kernel argument; slots ride in bytes; a row's distinct cells fit the lane's words");
// ONE launch for the n_units units of tab.  stats: five runs of n_units words: [u] += the source cells read at or above 2^32,
// [n_units + u] += the rows of check u with a cell that differs, [2 n_units + u] += the messages started, [3 n_units + u] <-
// min(., the smallest row of the first kind), [4 n_units + u] <- min(., of the second).  Sources are only read and may
// coincide; out must not overlap a source.  Returns without a launch on a table that the caller's checks should have refused
void launch_sha256(hipStream_t s, const ShaTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the Keccak-f[1600] permutation columns of kzg_rows_commit_keccak (fr_keccak.hip).  Every value is a 64-bit lane: the low 64
// bits of a source cell's canonical integer in, int_store's cell out; lane (x, y) of a state has the flat index x + 5 y.  Source
// vector d lies at src + d T 8 words.  A ROW unit runs one permutation per row t' < n: slot[j] of state lane j is an index into
// the unit's list ld of n_ld DISTINCT source vectors (each cell is loaded once) or KEC_IMM: then the lane is imm[j].  It writes
// lane col[c] of the permuted state to vector c < n_out of out; with out null it is a check and compares that lane with the cell
// of source vector exp[c].  A ROUNDS unit walks the blocks of `period` rows: ld[0 .. 4] are the message vectors (lane x + 5 y <
// rate of a block absorbs the cell of ld[x] at block row y), ld[5] the start vector (KEC_IMM: every block starts a message);
// bit i of nocount: the cell of absorbed lane i is counted by another reader of the same cell (an earlier lane of the same
// vector, or the start cell); it writes column id col[c] (KEC_COL_A + x, .., KEC_COL_B + x) to vector c < n_out of out, which
// the caller has zeroed
#define KEC_MAX_UNITS 4
#define KEC_ROW 1
#define KEC_ROUNDS 2
#define KEC_IMM 0xffu
#define KEC_MIN_PERIOD 125
#define KEC_N_COLS 25
#define KEC_MAX_OUT 16
#define KEC_LANE_WORDS 50   // LDS words per lane: 25 values of 64 bits: a ROW unit's loaded cells, then its permuted state; a
                            // ROUNDS unit's absorbed cells, then the 25 values of a stage
enum { KEC_COL_A = 0, KEC_COL_P = 5, KEC_COL_D = 10, KEC_COL_T = 15, KEC_COL_B = 20 };
struct KecUnit {
    uint32_t* out;
    uint32_t mode, period, n_out, n_ld, rate, nocount;
    uint64_t imm[25];
    uint8_t slot[25], ld[POLY_MAX_ROWS], col[KEC_MAX_OUT], exp[KEC_MAX_OUT];
};
struct KecTab {
    KecUnit u[KEC_MAX_UNITS];
    const uint32_t* src;
    uint32_t n_units;
};
static_assert(sizeof(KecTab) + 64 <= 4096 && POLY_MAX_ROWS < KEC_IMM && 2 * POLY_MAX_ROWS <= KEC_LANE_WORDS && POLY_MAX_ROWS >= 6,
              "the unit table rides as a kernel argument; slots ride in bytes; a row's distinct cells fit the lane's words");
// ONE launch for the n_units units of tab.  stats: five runs of n_units words: [u] += the source cells read at or above 2^64,
// [n_units + u] += the rows of check u with a cell that differs, [2 n_units + u] += the messages started, [3 n_units + u] <-
// min(., the smallest row of the first kind), [4 n_units + u] <- min(., of the second).  Sources are only read and may
// coincide; out must not overlap a source.  Returns without a launch on a table that the caller's checks should have refused
void launch_keccak(hipStream_t s, const KecTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the non-native elliptic-curve columns of kzg_rows_commit_ec (fr_ec.hip).  A wide value is `limbs` source vectors of `bits`
// bits each, little-endian, as in fr_wide.hip, at most 256 bits: EC_WORDS 32-bit words.  The curve is uniform over the call: the
// odd modulus p, the coefficient a < p, and what the Montgomery products of radix 2^256 need: n0inv = -p^-1 mod 2^32 and r2 =
// 2^512 mod p (the caller computes both).  Source vector d lies at src + d T 8 words.  slot[w][l]: the vector of limb l of operand
// w (DIV: a, b; ADD: x1, y1, x2, y2; CHAIN: px, py); opv: the vector of a CHAIN unit's op-code column.  cols: bit k set: name k
// (DIV: r; ADD: lam, x3, y3; CHAIN: ax, ay, lam) is an output, `limbs` vectors each, side by side at out in the order of the
// names.  out null: a check (DIV, ADD): limb l of name k is compared with the cell of source vector exp[k][l]
#define EC_MAX_UNITS 4
#define EC_MAX_LIMBS 4
#define EC_WORDS 8
#define EC_DIV 1
#define EC_ADD 2
#define EC_CHAIN 3
#define EC_F_IMM_B 0x100u   // DIV: operand b is imm
struct EcUnit {
    uint32_t* out;
    uint32_t mode, cols, flags, opv;
    uint8_t slot[4][EC_MAX_LIMBS], exp[3][EC_MAX_LIMBS];
    uint32_t imm[EC_WORDS];
};
struct EcTab {
    EcUnit u[EC_MAX_UNITS];
    const uint32_t* src;
    uint32_t n_units, bits, limbs, n0inv;
    uint32_t p[EC_WORDS], a[EC_WORDS], r2[EC_WORDS];
};
static_assert(sizeof(EcTab) + 64 <= 4096 && POLY_MAX_ROWS <= 256, "the unit table rides as a kernel argument; slots ride in bytes");
// ONE launch for the n_units units of tab.  stats: seven runs of n_units words: [u] += the rows with a limb at or above 2^bits
// or an operand at or above p, [n_units + u] += the exceptional (singular) rows, [2 n_units + u] += the rows of a check with a
// cell that differs, on a CHAIN unit the rows with an unknown op-code, [3 n_units + u] += the segments of a CHAIN unit, [4 n_units
// + u], [5 n_units + u], [6 n_units + u] <- min(., the smallest row of the first, second and third kind).  Sources are only read
// and may coincide; out must not overlap a source.  Returns without a launch on a table that the caller's checks should have
// refused (p even or below 3, a >= p, bits or limbs out of range, an unknown mode, no name)
void launch_ec(hipStream_t s, const EcTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// ---- the native twisted-Edwards columns of kzg_rows_commit_edwards (fr_edwards.hip).  A coordinate is one cell of source vector
// slot[w] (src + slot T 8 words; ADD: x1, y1, x2, y2; CHAIN: px, py) or, at EDW_IMM, the unit's immediate imm[w]; opv: the vector
// of a CHAIN unit's op-code column.  a, d and imm are canonical integers as 8 little-endian 32-bit words.  cols: bit k set: name k
// (ADD: x3, y3; CHAIN: ax, ay) is computed; out[k]: the vector it is written to (null: not written); q: the unit's slice of the
// denominator vector.  q null: a check (ADD): name k is compared with the cell of source vector exp[k]
#define EDW_MAX_UNITS 4
#define EDW_ADD 1
#define EDW_CHAIN 2
#define EDW_IMM 0xffu
struct EdwUnit {
    uint32_t *out[2], *q;
    uint32_t mode, cols, opv, reserved;
    uint8_t slot[4], exp[2], pad[2];
    uint32_t imm[4][8];
};
struct EdwTab {
    EdwUnit u[EDW_MAX_UNITS];
    const uint32_t* src;
    uint32_t n_units, reserved;
    uint32_t a[8], d[8];
};
static_assert(sizeof(EdwTab) + 64 <= 4096 && POLY_MAX_ROWS < EDW_IMM, "the unit table rides as a kernel argument; slots ride in bytes");
// ONE launch for the n_units units of tab, over all T rows: a committing unit leaves its numerators (ADD) or projective X, Y
// (CHAIN) in out[k] on the rows t < n and its denominators in q on ALL T rows, never zero (Montgomery 1 on an exceptional row
// and on the rows >= n).  stats: five runs of n_units words: [u] += the exceptional rows or steps, [n_units + u] += the rows of a
// check with a cell that differs, on a CHAIN unit the rows with an unknown op-code, [2 n_units + u] += the segments of a CHAIN
// unit, [3 n_units + u], [4 n_units + u] <- min(., the smallest row of the first and second kind).  Sources are only read and may
// coincide; out and q must not overlap a source.  Returns without a launch on a table that the caller's checks should have refused
void launch_edwards(hipStream_t s, const EdwTab& tab, uint64_t T, uint64_t n, uint64_t* stats);
// behind the inversion of the denominators: out[c T + t] <- out[c T + t] W[wq[c] T + t], canonical, for c < n_out and t < n
struct EdwFin {
    uint32_t* out;
    const uint32_t* W;
    uint8_t wq[POLY_MAX_ROWS];
};
void launch_edwards_finish(hipStream_t s, const EdwFin& fin, uint32_t n_out, uint64_t T, uint64_t n);
// ---- the expression columns of kzg_rows_commit_expr (fr_expr.hip): v[t] = sum_u c_u prod_f src.r[row[u][f]][(t + rot[u][f]) mod T]
// for t < n <= T over evaluation vectors of T canonical Montgomery elements (T a power of two, at most 2^32)
#define EXPR_MAX_TERMS 16
#define EXPR_MAX_FACTORS 8
struct ExprPlan {
    uint32_t n_terms;                                   // 1 .. EXPR_MAX_TERMS
    const uint8_t* coeffs_be32;                         // n_terms canonical scalars, 32 big-endian HOST bytes each (the caller's check)
    uint8_t term_len[EXPR_MAX_TERMS];                   // 0 .. EXPR_MAX_FACTORS
    uint8_t term_row[EXPR_MAX_TERMS][EXPR_MAX_FACTORS]; // index into src
    uint32_t term_rot[EXPR_MAX_TERMS][EXPR_MAX_FACTORS];// in [0, T)
};
// out (null: a check, nothing is stored) [t] <- v[t], canonical, for t < n; *nonzero += the cells t < n with v[t] != 0;
// *first <- min(*first, the smallest such t).  out must not alias a source (a rotated factor reads other cells)
void launch_expr(hipStream_t s, const RowTab& src, const ExprPlan& ep, uint32_t* out_or_null, uint64_t T, uint64_t n,
                 uint64_t* nonzero, uint64_t* first);
// ---- the first-order recurrence columns of kzg_rows_commit_recurrence (fr_recur.hip): v[0] = start, v[t + 1] = A[t] v[t] + B[t]
// for t < n over two vectors of canonical Montgomery elements, as a scan of affine maps.  "Plan, then run", as the opening scan:
// level 0 is the vectors themselves, level k folds chunks of 2^l[k] of its n[k] maps (2^l0 at level 0, 16 above) into level
// k + 1, which starts at element off[k + 1] of BOTH scratch arrays, until at most top_max maps are left for the one workgroup of
// the top kernel (K = 0: the vectors go to it directly).  recur_plan is what the launcher picks (l0 = 2 below 2^17, 3 below
// 2^18, else 4; RECUR_TOP_MAX), recur_plan_levels a caller's choice, recur_plan_invalid the kernels' preconditions (null:
// valid): l0 in 2 .. 4, 1 <= top_max <= RECUR_TOP_MAX, at most RECUR_MAX_LEVELS levels, the stacked levels inside
// recur_level_elems(n).  The overload that takes a plan runs it unchecked.
#define RECUR_TOP_MAX 2048
#define RECUR_MAX_LEVELS 14
struct RecurPlan {
    int l0, lup, K;
    uint64_t top_max;
    int l[16];
    uint64_t n[16], off[16];
};
// elements of EACH of the two scratch arrays: the stacked levels above level 0, sized as the other scans size theirs
inline uint64_t recur_level_elems(uint64_t n) { return poly_level_words(n) / 8; }
RecurPlan recur_plan(uint64_t n);
RecurPlan recur_plan_levels(uint64_t n, int l0, uint64_t top_max);
const char* recur_plan_invalid(const RecurPlan& pl, uint64_t n);
// out[t] <- v[t] for t < n (canonical; out must not alias A or B); closing_be (device) <- v[n] as 32 big-endian bytes;
// close_row (device, null: none) <- v[n] as a canonical Montgomery element.  A and B are only read; scrA, scrB:
// recur_level_elems(n) elements each; start_be32: a canonical scalar as 32 big-endian HOST bytes (the caller's check; a kernel
// argument).  1 <= n <= 2^32
void launch_recur_scan(hipStream_t s, const uint32_t* A, const uint32_t* B, uint64_t n, uint32_t* scrA, uint32_t* scrB,
                       const uint8_t start_be32[32], uint32_t* out, uint8_t* closing_be, uint32_t* close_row);
void launch_recur_scan(hipStream_t s, const RecurPlan& pl, const uint32_t* A, const uint32_t* B, uint64_t n, uint32_t* scrA,
                       uint32_t* scrB, const uint8_t start_be32[32], uint32_t* out, uint8_t* closing_be, uint32_t* close_row);
// the one level loop behind recur_plan_levels (min_levels = 0) and scan_plan_levels (1): levels are added while the top one
// holds more than top_max values or fewer than min_levels levels lie under it
RecurPlan ladder_plan_levels(uint64_t n, int l0, uint64_t top_max, int min_levels);
// ---- the plans of the product scan (fr_prod.hip: launch_gp_scan_upper, launch_gp_scan, and launch_fr_batch_inv of fr_lookup.hip
// behind it) and of the additive scan (fr_lookup.hip: launch_lk_sum_scan).  The ladder is the recurrence scan's, and so is the
// plan type, with ONE difference: these scans have no K = 0 form.  Level 0 (the vectors themselves, 2^l0 elements per lane) is
// always folded into level 1 at element 0 of the scratch, even at n = 1; levels of 16 follow while more than top_max values are
// left for the one workgroup of the top kernel.  scan_plan is what the launchers pick (l0 = 2, raised to 3 or 4 while
// (n >> (l0 + 1)) >= 16384; SCAN_TOP_MAX), scan_plan_levels a caller's choice, scan_plan_invalid the kernels' preconditions
// (null: valid): 1 <= n <= 2^32, l0 in 2 .. 4, 1 <= top_max <= SCAN_TOP_MAX, 1 .. SCAN_MAX_LEVELS levels, the stacked levels
// inside scan_level_elems(n).  The overloads that take a plan run it unchecked.
#define SCAN_TOP_MAX 2048
#define SCAN_MAX_LEVELS RECUR_MAX_LEVELS
typedef RecurPlan ScanPlan;
// elements of EACH scratch array: what every caller allocates ((n + 3) / 4 * 3 / 2 + 64)
inline uint64_t scan_level_elems(uint64_t n) { return poly_level_words(n) / 8; }
ScanPlan scan_plan(uint64_t n);
ScanPlan scan_plan_levels(uint64_t n, int l0, uint64_t top_max);
const char* scan_plan_invalid(const ScanPlan& pl, uint64_t n);
// what the launchers themselves ask before they launch: a plan of n elements with 1 .. SCAN_MAX_LEVELS levels and a top that
// one workgroup takes
bool scan_plan_runs(const ScanPlan& pl, uint64_t n);
// the launchers above by a caller's plan (theirs is scan_plan(n)); launch_gp_scan_upper answers -1, and nothing is launched by
// any of them, for a plan that is not of n elements or has no level table
int launch_gp_scan_upper(hipStream_t s, const ScanPlan& pl, const uint32_t* N, const uint32_t* D, uint64_t n, uint32_t* scrN,
                         uint32_t* scrD, uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32 = nullptr);
void launch_gp_scan(hipStream_t s, const ScanPlan& pl, uint32_t* N, uint32_t* D, uint64_t n, uint32_t* scrN, uint32_t* scrD,
                    uint8_t* closing_be, uint32_t* zero_flag, const uint8_t* start_be32 = nullptr);
void launch_fr_batch_inv(hipStream_t s, const ScanPlan& pl, const uint32_t* Q, uint32_t* W, const uint32_t* P_or_null,
                         uint32_t* out, uint64_t n, uint32_t* scrN, uint32_t* scrD, uint8_t* scratch32, uint32_t* zero_flag);
void launch_lk_sum_scan(hipStream_t s, const ScanPlan& pl, uint32_t* v, uint64_t n, uint32_t* scr, uint8_t* closing_be);
// ---- blinding rows (fr_blind.hip; the kzg_rows_commit_*_zk builders): rows [usable, n) of evaluation vectors of n Montgomery
// elements, n - usable <= BLIND_MAX_ROWS (= KZG_MAX_BLIND_ROWS)
#define BLIND_MAX_ROWS 32
// a[t] <- 1 (a_one) or 0, b[t] <- 1 for usable <= t < n: the neutral operands of the product scan / the running fraction
void launch_blind_mask(hipStream_t s, uint32_t* a, bool a_one, uint32_t* b, uint64_t n, uint64_t usable);
// v[usable + 1 + j] <- tail[j], j < n - usable - 1; tail_be32: that many canonical scalars as 32 big-endian HOST bytes each (a
// kernel argument; not read when usable = n - 1), *bad raised when one is >= r
void launch_blind_tail(hipStream_t s, uint32_t* v, uint64_t n, uint64_t usable, const uint8_t* tail_be32, uint32_t* bad);
