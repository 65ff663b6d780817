/* kzg_mi355x_scan_test.h -- the plan hooks of the product scan (csrc/fr_prod.hip, with the batched inversion of csrc/fr_lookup.hip
 * behind it) and of the additive scan (csrc/fr_lookup.hip): test hooks of libkzg_mi355x.so like those of kzg_mi355x_test.h, which
 * includes this file.  They are declared apart because tests/test_abi.py pins the exact list of the names that kzg_mi355x_test.h
 * itself declares; tests/test_scan_plans_cpu.py checks this file against the bindings.  Nothing here is part of the serving
 * surface.
 *
 * Both scans run as the same ladder of levels: level 0 is the vectors themselves and folds chunks of 2^l0 elements into level 1,
 * every level above it chunks of 16 values of the level below, until at most top_max values are left for the one workgroup of
 * the top kernel; the values then go back down level by level and a level-0 kernel writes the result.  UNLIKE the recurrence scan
 * there is no K = 0 form: level 0 is always folded once, so K >= 1 even at n = 1.  l0 = top_max = -1: the plan the library picks
 * for n (l0 = 2 below 2^17, 3 below 2^18, else 4; 2048).  Anything else: the CALLER'S plan, both as given.  A plan is checked
 * against the kernels' preconditions first, KZG_E_ARG with the reason in kzg_last_error otherwise:
 *   1 <= n <= 2^32; l0 in 2 .. 4; 1 <= top_max <= 2048; 1 .. 14 levels; the stacked level arrays inside the scratch the library
 *   allocates for n (ceil(n / 4) * 3 / 2 + 64 elements per array)
 * (with l0 and top_max in range no n <= 2^32 needs more than 9 levels, and the levels always fit: the last two refusals guard
 * the launchers against a plan built by other means).
 * kzg_test_scan_plan_of: host only, no context.  out_K: the levels K; out_l, out_n, out_off: room for 16 entries, K + 1 are
 * filled -- level k folds chunks of 2^l[k] of its n[k] values, kept from element off[k] of the scratch (level 0: the vectors
 * themselves, offset unused; level K: what the top kernel takes, l = 0).
 * kzg_test_scan_run: upload, the plan through the library's own launcher on the lane's level scratch, download -- no SRS, no
 * MSM.  The plan, and then the other arguments, are judged before the context is looked at.  a_be32, b_be32: n canonical scalars
 * each, 32 big-endian bytes (KZG_E_SCALAR otherwise); n <= 2^22.  form:
 *   0  launch_gp_scan, N = a, D = b:            out[t] = prod_{u<t} a[u] / b[u], closing = prod_u a[u] / b[u]
 *   1  the same with start_be32 (one scalar, canonical and not 0 as kzg_rows_commit_grand_product_chain asks, KZG_E_ARG
 *      otherwise): every out[t] and the closing value times start
 *   2  launch_fr_batch_inv, Q = a, no P, out = W (as the derived and the Edwards columns call it): out[t] = 1 / a[t]
 *   3  launch_fr_batch_inv, Q = a, P = b, out = P (as the lookup sum calls it):                    out[t] = b[t] / a[t]
 *   4  launch_lk_sum_scan in place on a:        out[t] = sum_{u<t} a[u], closing = sum_u a[u]
 * An operand that a form does not read may be NULL (b: forms 2 and 4; start: every form but 1).  out_be32: n x 32 bytes.  The
 * level scratch and W start from a fill pattern that is no scalar and the words come back without a reduction check, so an
 * element that no kernel wrote shows (forms 0, 1, 3 and 4 work in place: there it shows as its input).  out_closing_be32: the 32
 * bytes the scan leaves in its record -- forms 2 and 3: prod a / prod a = 1.  out_zero_flag: the scan's zero-denominator word
 * as the top kernel left it (forms 0 to 3; 1: some denominator is 0, the values are then unspecified and the call still
 * answers KZG_OK), 0 in form 4. */
#ifndef KZG_MI355X_SCAN_TEST_H
#define KZG_MI355X_SCAN_TEST_H
#include "kzg_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif
int kzg_test_scan_plan_of(uint64_t n, int l0, int64_t top_max, int* out_K, int* out_l, uint64_t* out_n, uint64_t* out_off);
int kzg_test_scan_run(kzg_ctx* ctx, int form, int l0, int64_t top_max, const uint8_t* a_be32, const uint8_t* b_be32,
                      const uint8_t* start_be32, uint64_t n, uint8_t* out_be32, uint8_t* out_closing_be32, uint32_t* out_zero_flag);
#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_SCAN_TEST_H */
