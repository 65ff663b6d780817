/* kzg_mi355x_recur_test.h -- the plan hooks of the recurrence scan (csrc/fr_recur.hip): test hooks of libkzg_mi355x.so like
 * those of kzg_mi355x_test.h, which includes this file.  They are declared apart because tests/test_abi.py pins the exact list
 * of the names that kzg_mi355x_test.h itself declares; tests/test_recurrence_cpu.py checks this file against the bindings.
 * Nothing here is part of the serving surface.
 *
 * v[0] = start, v[t + 1] = a[t] v[t] + b[t] for t < n runs as a ladder of levels over the affine maps (a[t], b[t]): level 0 is
 * the two vectors themselves and folds chunks of 2^l0 maps, every level above it chunks of 16 maps of the level below, until at
 * most top_max maps are left for the one workgroup of the top kernel (n <= top_max: K = 0 levels, the vectors go to it
 * directly); the values then go back down level by level and the level-0 walk writes v.  l0 = top_max = -1: the plan the
 * library picks for n (l0 = 2 below 2^17, 3 below 2^18, else 4; 2048).  Anything else: the CALLER'S plan, both as given.
 * A plan is checked against the kernels' preconditions first, KZG_E_ARG with the reason in kzg_last_error otherwise:
 *   1 <= n <= 2^32; l0 in 2 .. 4; 1 <= top_max <= 2048; at most 14 levels; the stacked level arrays inside the scratch the
 *   library allocates for n (ceil(n / 4) * 3 / 2 + 64 elements in each of the two arrays)
 * kzg_test_recur_plan_of: host only, no context.  out_K: the levels K; out_l, out_n, out_off: room for 16 entries, K + 1 are
 * filled -- level k folds chunks of 2^l[k] of its n[k] maps, kept from element off[k] of both scratch arrays (level 0: the
 * vectors themselves, offset unused; level K: what the top kernel takes, l = 0).
 * kzg_test_recur_run: upload, the plan through the library's own launcher, download -- no SRS, no MSM.  The plan (and then the
 * other arguments) are judged before the context is looked at.  a_be32, b_be32: n canonical scalars each, 32 big-endian bytes;
 * start_be32: one.  out_v_be32: n x 32 bytes, v[0] .. v[n - 1], written over a fill pattern that is no scalar;
 * out_closing_be32: v[n].  n <= 2^22. */
#ifndef KZG_MI355X_RECUR_TEST_H
#define KZG_MI355X_RECUR_TEST_H
#include "kzg_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif
int kzg_test_recur_plan_of(uint64_t n, int l0, int64_t top_max, int* out_K, int* out_l, uint64_t* out_n, uint64_t* out_off);
int kzg_test_recur_run(kzg_ctx* ctx, int l0, int64_t top_max, const uint8_t* a_be32, const uint8_t* b_be32,
                       const uint8_t start_be32[32], uint64_t n, uint8_t* out_v_be32, uint8_t* out_closing_be32);
#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_RECUR_TEST_H */
