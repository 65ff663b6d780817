// rows_impl.h -- the internal entries behind the row-set exports, declared ONCE for their two callers: serve.hip, which
// defines them and whose kzg_rows_* exports call them with expect_i = UINT32_MAX, and multi_host.cpp, whose kzg_multi_rows_*
// exports call them with the routed slice.  Plain C++17 over the public header: no HIP type appears here.
//
// Every entry takes the public call's arguments behind (ctx, expect_i).  expect_i is the one thing the public forms lack:
// every set (and accumulator) named must belong to worker `expect_i`; UINT32_MAX accepts any one worker.  A builder has ONE
// entry for all its variants: what a variant adds arrives as an optional argument (null: the variant without it).
#pragma once
#include "../../include/kzg_mi355x.h"

namespace kzg_impl {

// The blinding rows of a kzg_rows_commit_*_zk builder (checked by the caller: 1 <= usable < T, T - usable <=
// KZG_MAX_BLIND_ROWS, every tail scalar canonical): rows [0, usable) carry the circuit, row `usable` closes the running value
// and rows usable + 1 .. T - 1 take the T - usable - 1 scalars of tail_be32 (host bytes).  Null: the plain builder.
struct Blind {
    uint64_t usable;
    const uint8_t* tail_be32;
};
// The selector arguments of a _sel builder as the caller gave them (null: the call has none): sel_index[l] is KZG_NO_SELECTOR
// or indexes the concatenated rows of the sel_handles sets, which must be of the call's worker and row length.  A _sel call
// always comes with a Blind: usable == T with no tail is the plain layout, decided once T is known.
struct SelCall {
    uint32_t n_sel_handles;
    const uint64_t* sel_handles;
    const uint32_t* sel_index;
};

int rows_open(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
              const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
              uint8_t* out_proofs48);
int rows_eval(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
              const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32);
int rows_lincomb(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                 const uint8_t* points_be32, const uint8_t* coeffs_be32, uint8_t* out_values32, uint8_t* out_proofs48);
int rows_shplonk(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                 const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32, uint8_t* out_commitment48,
                 uint64_t* out_handle);
int rows_release(kzg_ctx* ctx, uint32_t expect_i, uint64_t handle);
int rows_read(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first,
              uint64_t count, uint32_t kind, int evaluation_form, void* out, uint64_t* out_overflow);
// zk: the blinding rows of the _zk and _chain calls.  start_be32: the _chain call's start of z (null: not a chain, z starts at 1)
int rows_grand_product(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                       uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k, const uint8_t* shifts_be32,
                       const uint8_t* beta_be32, const uint8_t* gamma_be32, uint8_t* out_commitment48, uint8_t* out_closing32,
                       uint64_t* out_handle, const Blind* zk, const uint8_t* start_be32);
// opts: the selectors and the blinding rows as the public call takes them (null: neither)
int rows_shuffle(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                 uint32_t n_shuffle_handles, const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width,
                 const uint8_t* theta_be32, const uint8_t* gamma_be32, const kzg_shuffle_opts* opts, uint8_t* out_commitment48,
                 uint8_t* out_closing32, uint64_t* out_handle);
// opts: the usable layout and its tail as the public call takes them (null: all T rows are sorted)
int rows_sorted(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t width,
                uint32_t n_keys, const kzg_sorted_opts* opts, uint8_t* out_commitments48, uint64_t* out_handle);
// opts: the usable layout and the free label as the public call takes them (null: all T rows take part, no free label)
int rows_sigma(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
               const uint8_t* shifts_be32, const kzg_sigma_opts* opts, uint8_t* out_commitments48, uint64_t* out_stats,
               uint64_t* out_handle);
int rows_check_copies(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                      uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts,
                      uint64_t* out);
// opts: the usable layout and its tail as the public call takes them (null: all T rows are read)
int rows_derived(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                 const kzg_derive_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
                 uint64_t* out_handle);
// opts: as for rows_derived
int rows_int(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
             const kzg_int_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
             uint64_t* out_first, uint64_t* out_handle);
// opts: as for rows_derived
int rows_alu(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_entries,
             const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units, const kzg_derive_opts* opts,
             uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_unknown,
             uint64_t* out_first_unknown, uint64_t* out_handle);
// opts: as for rows_derived
int rows_wide(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
              const kzg_wide_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
              uint64_t* out_first, uint64_t* out_qover, uint64_t* out_first_qover, uint64_t* out_handle);
// opts: as for rows_derived
int rows_poseidon(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                  const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units, const kzg_derive_opts* opts,
                  uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                  uint64_t* out_handle);
// opts: as for rows_derived
int rows_poseidon2(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                   const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                   const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_mismatch,
                   uint64_t* out_first_mismatch, uint64_t* out_handle);
// opts: as for rows_derived
int rows_sha256(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                const kzg_sha256_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_blocks,
                uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_mismatch,
                uint64_t* out_first_mismatch, uint64_t* out_handle);
// opts: as for rows_derived
int rows_keccak(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                const kzg_keccak_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_mismatch,
                uint64_t* out_first_mismatch, uint64_t* out_handle);
// opts: as for rows_derived.  out_stats: the nine statistics arrays of kzg_rows_commit_ec in the order of its arguments
int rows_ec(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, const kzg_ec_curve* curve,
            uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
            uint64_t* const out_stats[9], uint64_t* out_handle);
// opts: as for rows_derived.  out_stats: the seven statistics arrays of kzg_rows_commit_edwards in the order of its arguments
int rows_edwards(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                 const kzg_edwards_curve* curve, uint32_t n_units, const kzg_edwards_unit* units, const kzg_derive_opts* opts,
                 uint8_t* out_commitments48, uint64_t* const out_stats[7], uint64_t* out_handle);
// opts: as for rows_derived.  out_stats: the six statistics arrays of kzg_rows_commit_poseidon_chain in the order of its arguments
int rows_poseidon_chain(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                        const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_chain_unit* units,
                        const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* const out_stats[6], uint64_t* out_handle);
// opts: the usable layout and its tail as the public call takes them (null: all T rows are evaluated)
int rows_expr(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_exprs,
              const kzg_expr* exprs, const kzg_expr_opts* opts, uint8_t* out_commitments48, uint64_t* out_nonzero,
              uint64_t* out_first, uint64_t* out_handle);
// opts: the usable layout (with a closing row) and its tail as the public call takes them (null: the plain layout)
int rows_recurrence(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_recs,
                    const kzg_recurrence* recs, const kzg_recurrence_opts* opts, uint8_t* out_commitments48,
                    uint8_t* out_closings32, uint64_t* out_handle);
// flags: 0 or KZG_FETCH_INDEX.  opts: the usable layout and its tail as the public call takes them (null: all T rows are read)
int rows_fetch(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
               const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys, uint32_t flags, const kzg_derive_opts* opts,
               uint8_t* out_commitments48, uint64_t* out_missing, uint64_t* out_first_missing, uint64_t* out_handle);
// zk: the blinding rows of the _zk call, the layout of the _sel call.  sc: the selectors of the _sel call
int rows_lookup_sum(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                    uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle, uint32_t n_lookups,
                    uint32_t width, const uint8_t* theta_be32, const uint8_t* beta_be32, uint8_t* out_commitment48,
                    uint8_t* out_closing32, uint64_t* out_handle, const Blind* zk, const SelCall* sc);
int rows_multiplicities(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                        uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                        uint8_t* out_commitment48, uint64_t* out_missing, uint64_t* out_handle, const Blind* zk,
                        const SelCall* sc);
// lookup: the _ext call's.  selectors: the _sel call's.  active: the _zk call's column A.  plain: the call came through
// kzg_rows_commit_quotient (quotient_plain_terms below), which only words one message
int rows_quotient(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                  const kzg_quotient_perm* perm, const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                  const kzg_quotient_active* active, uint32_t ext_log, uint32_t n_pieces, uint8_t* out_commitments48,
                  uint64_t* out_handle, bool plain);
int rows_quotient_part(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles,
                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                       const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                       const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32, uint64_t* inout_acc);
int rows_quotient_finish(kzg_ctx* ctx, uint32_t expect_i, uint64_t acc, uint32_t n_pieces, uint8_t* out_commitments48,
                         uint64_t* out_handle);

// kzg_rows_commit_quotient's gate as the terms of the general call: every rotation 0 (the caller has checked gate != NULL)
inline kzg_quotient_terms quotient_plain_terms(const kzg_quotient_gate* gate) {
    return {gate->n_terms, gate->coeffs_be32, gate->term_lens, gate->term_rows, nullptr};
}

}  // namespace kzg_impl
