/* kzg_mi355x_test.h -- test hooks of libkzg_mi355x.so: the SAME library, a separate declaration.
 *
 * Nothing here is part of the serving surface (include/kzg_mi355x.h): these entry points expose single field / group /
 * pairing operations and the host-side point encoder so that tests/test_gpu_*.py, tests/test_abi.py and
 * tests/test_verify.py can compare each of them with the oracle.  A binding of the prover never needs
 * this file.
 *
 * The hooks, in the order of this file: unit operations (kzg_test_field, kzg_test_g1), raw limbs (kzg_test_fp_raw,
 * kzg_test_g1_raw), the NTT's pass plans (kzg_test_ntt_plan_of, kzg_test_ntt_run), the opening scan's plans
 * (kzg_test_poly_plan_of, kzg_test_poly_run), the hash join (kzg_test_join, kzg_test_join_counts), the MSM's passes
 * (kzg_test_msm_passes), the host-side encoder (kzg_host_xyzz_*), the communicator stall (kzg_test_comm_stall, _n), the pairing
 * (kzg_vk_pairing); and,
 * declared in files of their own that this one includes at its end, the recurrence scan's plans (kzg_mi355x_recur_test.h:
 * kzg_test_recur_plan_of, kzg_test_recur_run) and the product and additive scans' plans (kzg_mi355x_scan_test.h:
 * kzg_test_scan_plan_of, kzg_test_scan_run).
 */
#ifndef KZG_MI355X_TEST_H
#define KZG_MI355X_TEST_H
#include "kzg_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- unit-op hooks for the parity tests (tests/test_gpu_units.py); not part of the serving surface */
int kzg_test_field(kzg_ctx* ctx, int field /*0 Fp,1 Fr*/, int op /*0 mul,1 add,2 sub,3 mul(plain C ref),4 sqr; Fr only: 7 a^-1 by the
                   device-side inversion of the grand-product call, giving 0 for a = 0; 8 that inversion's zero flag, 0 or 1; 9 a^-1 for all n
                   elements by the batched inversion of the lookup-sum call (one device-side inversion in all), KZG_E_ARG when
                   some a = 0; b unused*/,
                   const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be, uint64_t n);
int kzg_test_g1(kzg_ctx* ctx, int op /*0 a+b mixed,1 2a+b full,2 2a,3 4a,4 a+20a+20b chain; lane-parallel forms: 5 2a+b,
                                         6 4a, 7 ten rounds r <- 2r+b from a*/, const uint8_t* a_be96,
                const uint8_t* b_be96, uint8_t* out_be96, uint64_t n);

/* ---- raw-limb hooks (tests/test_gpu_fp_classes.py, reference tests/fp28_ref.py): operands and results are the working limbs
 * themselves -- 14 words of 28 bits per Fp element (field 0), 9 words of 29 bits per Fr element (field 1) -- with no conversion, no
 * Montgomery entry or exit and no canonicalisation beyond what the operation does itself, so that a test can place every operand on
 * the bounds of its representation class.  An operand that the operation does not read may be NULL.
 *   field 0: 0 fp_mul(a, b), 1 fp_mul_inline, 2 fp_sqr(a), 3 fp_sqr_inline, 4 fp_mul2_inline(a, b, c, d), 5 / 6 / 7 fp_sub4 / fp_sub8 /
 *            fp_sub16(a, b) then fp_norm, 8 fp_neg8(a), 9 fp_canon, 10 fp_canon_mont, 11 fp_neg_canon, 12 fp_is_zero_n (the answer in
 *            limb 0, the other limbs zero); lane-parallel, four elements per wave, one per DPP row: 13 lp_mul(a, b), 14 lp_norm of the
 *            14 lane values a (low words) | b (high words) << 32
 *   field 1: 0 fr9_mul(a lazy, b), 1 fr9_sub4(a, b), 2 fr9_sub8(a, b) (both as they leave, not normalised), 3 fr9_norm(a),
 *            4 fr9_reduce(a), 5 fr9_reduce_approx(a) */
int kzg_test_fp_raw(kzg_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                    uint32_t* out, uint64_t n);
/* points on raw XYZZ coordinates: 4 x 14 words per operand (X, Y, ZZ, ZZZ; all zero = infinity); the mixed additions read b's first
 * 28 words as the canonical affine x, y.  The result is the affine point, 96 big-endian bytes (zeros = infinity).
 *   0 g1_add<false>, 1 g1_add<true> (inlined products, paired reduction), 2 g1_madd<false>, 3 g1_madd<true>, 4 g1_dbl(a),
 *   5 lp_add, 6 lp_dbl(a) (one wave per element) */
int kzg_test_g1_raw(kzg_ctx* ctx, int op, const uint32_t* a_xyzz, const uint32_t* b_xyzz, uint8_t* out_be96, uint64_t n);

/* ---- the NTT's pass plans (tests/test_ntt_plans_cpu.py, tests/test_gpu_ntt_plans.py, reference tests/ntt_ref.py).  A transform
 * of 2^log_n elements is `passes` launches of one kernel form; pass p runs S[p] butterfly stages on tiles of 2^S[p] rows x
 * 2^logC[p] columns.
 * kzg_test_ntt_plan_of: the plan the library itself runs, host only, no context.  kernel -1: the form it picks for this size
 * (radix-2 below 2^18, or everywhere under KZG_NTT_RADIX2=1), 0: the register-blocked form, 1: the radix-2 form, whatever the
 * size; tile_log 0: the tile it uses (KZG_NTT_TILE_LOG, or 10), 8 .. 11: that tile (the radix-2 form has one tile, 10).
 * log_n in [1, 31].  out_S, out_logC: room for 8 passes.  Returns the form (0 register-blocked, 1 radix-2) or KZG_E_ARG.
 * kzg_test_ntt_run: kzg_ntt's path (upload, twiddles, scratch, launches, download) with the CALLER'S plan in place of the
 * library's; kernel 0 or 1, log_n in [1, 22], at most 8 passes.  The plan is checked against the kernels' preconditions before
 * anything is launched (and before the context is looked at), KZG_E_ARG with the reason in kzg_last_error otherwise:
 *   sum S = log_n, every S >= 1; radix-2: S <= 8 and S + logC <= 10; register-blocked: S <= 9 and S + logC <= 11;
 *   logC >= 0; first pass: logC <= log_n - S; later passes: logC <= s0 = the sum of the earlier S */
int kzg_test_ntt_plan_of(int log_n, int kernel, int tile_log, int* out_S, int* out_logC, int* out_passes);
int kzg_test_ntt_run(kzg_ctx* ctx, uint8_t* inout_be32, int log_n, int inverse, int kernel, int passes, const int* S,
                     const int* logC);

/* ---- the opening scan's plans (tests/test_poly_plans_cpu.py, tests/test_gpu_poly_plans.py, reference tests/poly_ref.py).
 * y = f(alpha) and q = (f - y) / (X - alpha) over n coefficients run as a ladder of levels: level 0 folds chunks of 2^l0
 * coefficients, every level above it chunks of 16 values of the level below, until at most scan_max values are left for one
 * workgroup of scan_nt lanes; the suffix values then go back down level by level and the division kernel (strided, or with
 * lds = 1 the LDS-staged one) writes q.  l0 = scan_max = scan_nt = lds = -1: the plan the library picks for n (l0 = 2 below 2^17,
 * 3 below 2^18, else 4; 2048; 1024 lanes for a top level of more than 1024 values; the LDS-staged division from 2^21 on multiples of
 * 1024, as KZG_POLY_NO_LDS / KZG_POLY_LDS_MIN_LOG move it).  Anything else: the CALLER'S plan, every parameter as given.
 * A plan is checked against the kernels' preconditions first, KZG_E_ARG with the reason in kzg_last_error otherwise:
 *   n >= 1; l0 in 2 .. 4; scan_max >= 1; scan_nt 256 or 1024; at most 14 levels; lds only with l0 = 4, n >= 1024 and
 *   n % 1024 == 0; the stacked level arrays inside the scratch the library allocates for n (ceil(n / 4) * 3 / 2 + 64 elements)
 * kzg_test_poly_plan_of: host only, no context.  out_K: the levels K; out_l, out_sq, out_n, out_off: room for 16 entries, K + 1
 * are filled -- level k folds chunks of 2^l[k] of its n[k] values, each weighing alpha^(2^sq[k]), kept from entry off[k] of the
 * scratch (level 0: the coefficients themselves; level K: what the scan takes, l = 0); out_scan_nt, out_lds: as run.
 * kzg_test_poly_run: upload, the plan through the library's own launcher, download -- no SRS, no MSM.  The plan (and then the
 * other arguments) are judged before the context is looked at.  f_be32: rows x n scalars, 32 big-endian bytes each; f_mont != 0:
 * they are Montgomery residues already and are stored as they are.  alphas_be32: nalphas points.  out_y_be32: one evaluation of 32
 * bytes per row (form 3: per pair).  out_q_words (forms 0, 4, 5): rows x n x 8 words, the buffer of q as the kernel left it
 * over a fill pattern -- n - 1 coefficients and the zero of slot n - 1 per row.  rows * n <= 2^22.  form:
 *   0 launch_poly_open, alpha as the first kernel's argument, q written         1 alpha read from memory, no q (rows = 1)
 *   2 launch_poly_eval_rows: rows <= 16 rows side by side at one point
 *   3 launch_poly_eval_pairs: pair t = row pair_row[t] at point pair_pt[t], npairs <= 64 point-major pairs over rows <= 16 rows that
 *     the hook lays out apart from each other and in descending order, nalphas <= 4 points
 *   4 launch_poly_open_points: rows <= 4 vectors, vector p at point p (nalphas = rows), canonical q
 *   5 the same with vector p at point pts[p] and q left in Montgomery form (the chained division of
 *     kzg_rows_commit_shplonk; always the strided kernel) */
int kzg_test_poly_plan_of(uint64_t n, int l0, int64_t scan_max, int scan_nt, int lds, int* out_K, int* out_l, int* out_sq,
                          uint64_t* out_n, uint64_t* out_off, int* out_scan_nt, int* out_lds);
int kzg_test_poly_run(kzg_ctx* ctx, int form, int l0, int64_t scan_max, int scan_nt, int lds, const uint8_t* f_be32, uint64_t n,
                      uint32_t rows, int f_mont, const uint8_t* pair_row, const uint8_t* pair_pt, uint32_t npairs,
                      const uint8_t* pts, const uint8_t* alphas_be32, uint32_t nalphas, uint8_t* out_y_be32,
                      uint32_t* out_q_words);

/* ---- the hash join alone (tests/test_join_cpu.py, tests/test_gpu_join.py, reference tests/join_ref.py): the open-addressing
 * table behind kzg_rows_commit_multiplicities, _zk, _sel and kzg_rows_commit_fetch, through the library's own launchers, with the
 * CALLER'S capacity in place of the builders' 2 T -- no SRS, no transform, no MSM.  The cells are canonical 32-byte big-endian
 * scalars, column-major, and are laid out as the builders lay them out (T elements of 8 canonical Montgomery words per column):
 *   tab_be32: (w + n_pay) x T, the w key columns first; in_be32: w x T, the cells of ONE lookup or read; sel_be32: T, the lookup's
 *   selector column (walk 2, NULL otherwise)
 *   build 0 launch_join_build, 1 launch_join_build_rows; walk 0 launch_join_probe, 1 _probe_rows, 2 _probe_sel, 3 launch_join_fetch
 * The arguments are judged before the context is looked at, KZG_E_ARG with the reason in kzg_last_error otherwise:
 *   1 <= rows <= T <= 2^12, rows = T for build 0 and for walk 0 (they take every row); cap a power of two, rows <= cap <= 2^12;
 *   w >= 1, w + n_pay <= 16; index 0 or 1 and only with walk 3, which needs n_pay + index >= 1; sel_be32 with walk 2 and only then
 * cap = rows with rows distinct tuples is a FULL table: a walk for an absent tuple then ends at its bound of cap steps, raises
 * *out_overrun and counts no miss (the builders turn that word into an error; cap = 2 T never gets there).
 * out_slots: the cap slot words after the build (a table row, or 2^32 - 1 for an empty slot); out_home: 2 T words, the slot at
 * which the walk of table row t starts, then that of cell t; out_cnt: the T counters (all zero after walk 3); out_fetch_be32 (walk
 * 3): (index + n_pay) x T cells, the index column first, cells at and behind `rows` as an unwritten fill pattern reads;
 * out_missing, out_first (2^64 - 1: none; walk 3 only), out_overrun: the walks' status words.
 * kzg_test_join_counts: launch_join_counts over n <= 2^12 caller-given counter words; out_be32: n canonical scalars. */
int kzg_test_join(kzg_ctx* ctx, int build, int walk, const uint8_t* tab_be32, const uint8_t* in_be32, const uint8_t* sel_be32,
                  uint64_t T, uint64_t rows, uint32_t w, uint32_t n_pay, int index, uint32_t cap, uint32_t* out_slots,
                  uint32_t* out_home, uint32_t* out_cnt, uint8_t* out_fetch_be32, uint64_t* out_missing, uint64_t* out_first,
                  uint32_t* out_overrun);
int kzg_test_join_counts(kzg_ctx* ctx, const uint32_t* cnt, uint64_t n, uint8_t* out_be32);

/* ---- the MSM passes of a multi-row call (tests/test_msm_passes_cpu.py): how the library splits k row sets + m tail sets (what
 * the openings divide out, one scalar set per point) at window c (2^(c-1) buckets per set) into passes of its Pippenger pipeline; long_rows: rows past the
 * length up to which sets share a pass (2^18).  Host only, no context.  out5: 5 words per pass, room for k + m passes -- first
 * row, rows, first tail set, tail sets, lane (0 the call's own, 1 its second).  c in [4, 24], k <= 16, m <= 4, else KZG_E_ARG. */
int kzg_test_msm_passes(int c, int long_rows, uint32_t k, uint32_t m, uint32_t* out5, int* out_passes);

/* the host encoder itself (no GPU): 4 x 14 limbs of 28 bits (X, Y, ZZ, ZZZ; lazy limbs < 2^32; residues with
 * R = 2^392) -> 48-byte compressed point / 192-byte partial record.  Test hooks. */
int kzg_host_xyzz_to_c48(const uint32_t xyzz_limbs28[56], uint8_t out48[48]);
int kzg_host_xyzz_pair_to_c48(const uint32_t a_limbs28[56], const uint32_t b_limbs28[56], uint8_t out_a48[48],
                              uint8_t out_b48[48]); /* two points, one shared inversion (commit + open) */
int kzg_host_xyzz_to_partial192(const uint32_t xyzz_limbs28[56], uint8_t out192[192]);

/* test hook for the timeout path of kzg_msm_sharded: the NEXT sharded MSM on this context first queues a kernel that
 * spins for `ms` milliseconds (bounded: at most 2000) on its lane, so that a 1-rank communicator can be made to overrun
 * kzg_comm_set_timeout without a dead peer. */
int kzg_test_comm_stall(kzg_ctx* ctx, int ms);
/* the same for the next `count` sharded MSMs (two calls in flight on two lanes: one times out, the other must not return a
 * result computed under the aborted communicator) */
int kzg_test_comm_stall_n(kzg_ctx* ctx, int ms, int count);

/* test hook: final_exp(miller(P, Q)) as 12 x 48 B in tower order (Fp12 = Fp6[w], Fp6 = Fp2[v], Fp2 = Fp[u]) */
int kzg_vk_pairing(const uint8_t p_be96[96], const uint8_t q_be192[192], uint8_t out_fp12[576]);

#ifdef __cplusplus
}
#endif
/* the plan hooks of the recurrence scan (csrc/fr_recur.hip), declared in a file of their own */
#include "kzg_mi355x_recur_test.h"
/* the plan hooks of the product scan and of the additive scan (csrc/fr_prod.hip, csrc/fr_lookup.hip), likewise */
#include "kzg_mi355x_scan_test.h"
#endif /* KZG_MI355X_TEST_H */
