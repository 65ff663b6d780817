"""ctypes binding of libkzg_mi355x.so (include/kzg_mi355x.h).  The HIP library IS the product: if it is
missing or no gfx950 device works, everything here raises -- there is no CPU fallback."""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# Eight hardware queues instead of the HIP runtime's four, unless the user chose: the four lanes of a context then run
# concurrently whatever the creation order of the process's streams (measured: profiles/r05_ab_hw_queues.log).  The runtime
# reads the variable once, at its first call -- so it is set HERE, when this module is imported: before the package starts
# a thread or touches HIP.  The library itself never writes the environment; it measures what it got (kzg_runtime_info) and
# `Client.start` warns when the lanes do not overlap (HIP was initialised earlier by somebody else, or the user chose fewer).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# KZG_MI355X_LIB: another BUILD of the same library (A/B candidates under zkp_subnet_amd/ab/, the prototype build): dev
# scripts point at it instead of overwriting the shipped file.  Never a different implementation, never a fallback.
LIB_PATH = os.environ.get("KZG_MI355X_LIB") or os.path.join(HERE, "libkzg_mi355x.so")

KZG_MAX_BATCH_OPEN = 16   # include/kzg_mi355x.h
KZG_MAX_OPEN_POINTS = 4
KZG_MAX_ROW_SETS = 64
KZG_MAX_SHPLONK_POINTS = 8                      # kzg_rows_commit_shplonk
KZG_MAX_SHPLONK_ROWS = KZG_MAX_BATCH_OPEN - 1   # round B opens k + 1 rows
KZG_MAX_GATE_TERMS = 16   # kzg_rows_commit_quotient
KZG_MAX_BLIND_ROWS = 32   # kzg_rows_commit_*_zk: T - usable
KZG_NO_SELECTOR = 0xffffffff   # kzg_rows_commit_*_sel: a lookup without a selector row
KZG_DERIVE_INV0, KZG_DERIVE_LIMBS = 1, 2   # kzg_rows_commit_derived: kzg_derive_op.kind
# kzg_rows_commit_int: kzg_int_op.kind, the immediate flag, out_first without an out-of-range cell
KZG_INT_AND, KZG_INT_OR, KZG_INT_XOR, KZG_INT_ADD, KZG_INT_SUB, KZG_INT_MUL, KZG_INT_DIVMOD, KZG_INT_SPLIT = range(1, 9)
KZG_INT_IMM = 1
KZG_INT_NONE = 0xffffffffffffffff
# kzg_rows_commit_alu: kzg_alu_entry.kind (the first eight are the KZG_INT_* kinds), the immediate flag, the sentinel, the limits
(KZG_ALU_AND, KZG_ALU_OR, KZG_ALU_XOR, KZG_ALU_ADD, KZG_ALU_SUB, KZG_ALU_MUL, KZG_ALU_DIVMOD, KZG_ALU_SPLIT, KZG_ALU_LTU,
 KZG_ALU_LT, KZG_ALU_EQ, KZG_ALU_SLL, KZG_ALU_SRL, KZG_ALU_SRA, KZG_ALU_ROTL, KZG_ALU_ROTR, KZG_ALU_MULHU, KZG_ALU_MULH,
 KZG_ALU_MULHSU, KZG_ALU_DIV, KZG_ALU_REM, KZG_ALU_REMU, KZG_ALU_SEXT) = range(1, 24)
KZG_ALU_IDLE = 0
KZG_ALU_IMM = 1
KZG_ALU_NONE = 0xffffffffffffffff
KZG_ALU_MAX_PROGRAM, KZG_ALU_MAX_UNITS = 64, 8
# kzg_rows_commit_wide: kzg_wide_op.kind, the flags, an operand field without a row, the limits
KZG_WIDE_ADD, KZG_WIDE_SUB, KZG_WIDE_MUL, KZG_WIDE_DIVMOD, KZG_WIDE_MULMOD, KZG_WIDE_CARRY = range(1, 7)
KZG_WIDE_IMM_B, KZG_WIDE_NEG_C = 1, 2
KZG_WIDE_ABSENT = 0xffffffff
KZG_WIDE_MAX_OPS, KZG_WIDE_MAX_LIMBS = 8, 8
# kzg_rows_commit_poseidon: kzg_poseidon_unit.mode, the flag, a slot that holds an immediate, "no mismatch", the limits
KZG_POSEIDON_ROW, KZG_POSEIDON_ROUNDS = 1, 2
KZG_POSEIDON_CHECK = 1
KZG_POSEIDON_IMM = 0xffffffff
KZG_POSEIDON_NONE = 0xffffffffffffffff
KZG_POSEIDON_MIN_T, KZG_POSEIDON_MAX_T = 2, 8
KZG_POSEIDON_MAX_FULL, KZG_POSEIDON_MAX_PARTIAL, KZG_POSEIDON_MAX_UNITS = 16, 128, 8
# kzg_rows_commit_poseidon2: the allowed widths (bit t set) and the limits; units, flags and "none" are kzg_rows_commit_poseidon's
KZG_POSEIDON2_WIDTHS = 0x11c
KZG_POSEIDON2_MAX_FULL, KZG_POSEIDON2_MAX_PARTIAL, KZG_POSEIDON2_MAX_UNITS = 16, 128, 8
# kzg_rows_commit_poseidon_chain: kzg_poseidon_chain_unit.mode, the flag, the layouts, "no such entry", the column ids of a flat
# unit (in_j, out_j), the limit; immediates and "none" are KZG_POSEIDON_IMM and KZG_POSEIDON_NONE
KZG_POSEIDON_CHAIN_SPONGE, KZG_POSEIDON_CHAIN_PATH = 1, 2
KZG_POSEIDON_CHAIN_CHECK = 1
KZG_POSEIDON_CHAIN_TRACE, KZG_POSEIDON_CHAIN_FLAT = 1, 2
KZG_POSEIDON_CHAIN_ABSENT = 0xffffffff
KZG_POSEIDON_CHAIN_COL_IN, KZG_POSEIDON_CHAIN_COL_OUT = 0, 8
KZG_POSEIDON_CHAIN_MAX_UNITS = 4
# kzg_rows_commit_sha256: kzg_sha256_unit.mode, the flags, a slot that holds an immediate, "no start column", "none", the limits,
# and the column ids of a rounds unit in the order of KZG_SHA256_COL_W .. KZG_SHA256_COL_CH
KZG_SHA256_ROW, KZG_SHA256_ROUNDS = 1, 2
KZG_SHA256_CHECK, KZG_SHA256_STD_IV = 1, 2
KZG_SHA256_IMM = 0xffffffff
KZG_SHA256_ABSENT = 0xffffffff
KZG_SHA256_NONE = 0xffffffffffffffff
KZG_SHA256_MAX_UNITS, KZG_SHA256_MIN_PERIOD, KZG_SHA256_N_COLS = 4, 72, 12
KZG_SHA256_COLS = ("w", "a", "e", "cw", "ca", "ce", "sig0", "sig1", "sum0", "maj", "sum1", "ch")
# kzg_rows_commit_keccak: kzg_keccak_unit.mode, the flag, a slot that holds an immediate, "no start column", "none", the limits,
# and the column names of a rounds unit in the order of their ids: KZG_KECCAK_COL_A + x, _P, _D, _T, _B
KZG_KECCAK_ROW, KZG_KECCAK_ROUNDS = 1, 2
KZG_KECCAK_CHECK = 1
KZG_KECCAK_IMM = 0xffffffff
KZG_KECCAK_ABSENT = 0xffffffff
KZG_KECCAK_NONE = 0xffffffffffffffff
KZG_KECCAK_MAX_UNITS, KZG_KECCAK_MIN_PERIOD, KZG_KECCAK_MAX_OUT, KZG_KECCAK_N_COLS = 4, 125, 16, 25
KZG_KECCAK_COLS = tuple(f"{k}{x}" for k in "apdtb" for x in range(5))
# kzg_rows_commit_ec: kzg_ec_unit.mode, the flags, "no such operand", "none", the limits, and the names of a unit's columns in
# the order of their bits in kzg_ec_unit.cols
KZG_EC_DIV, KZG_EC_ADD, KZG_EC_CHAIN = 1, 2, 3
KZG_EC_CHECK, KZG_EC_IMM_B = 1, 2
KZG_EC_ABSENT = 0xffffffff
KZG_EC_NONE = 0xffffffffffffffff
KZG_EC_MAX_UNITS, KZG_EC_MAX_LIMBS = 4, 4
KZG_EC_ADD_NAMES = ("lam", "x3", "y3")
KZG_EC_CHAIN_NAMES = ("ax", "ay", "lam")
# kzg_rows_commit_edwards: kzg_edwards_unit.mode, the flag, a slot that holds an immediate, "no such entry", "none", the limit, and
# the names of a unit's columns in the order of their bits in kzg_edwards_unit.cols
KZG_EDWARDS_ADD, KZG_EDWARDS_CHAIN = 1, 2
KZG_EDWARDS_CHECK = 1
KZG_EDWARDS_IMM = 0xfffffffe
KZG_EDWARDS_ABSENT = 0xffffffff
KZG_EDWARDS_NONE = 0xffffffffffffffff
KZG_EDWARDS_MAX_UNITS = 4
KZG_EDWARDS_ADD_NAMES = ("x3", "y3")
KZG_EDWARDS_CHAIN_NAMES = ("ax", "ay")
KZG_MAX_EXPR_FACTORS = 8   # kzg_rows_commit_expr: factors of one term
KZG_EXPR_CHECK = 1   # kzg_expr.flags: evaluate and count only
KZG_EXPR_NONE = 0xffffffffffffffff   # out_first: no non-zero cell
KZG_FETCH_INDEX = 1   # kzg_rows_commit_fetch flags: lead every read's outputs with the matching row number
KZG_FETCH_NONE = 0xffffffffffffffff   # out_first_missing: no miss
KZG_COL_BE32, KZG_COL_U8, KZG_COL_U16, KZG_COL_U32, KZG_COL_U64, KZG_COL_I32, KZG_COL_I64 = range(7)   # kzg_col.kind
KZG_READ_NONE = 0xffffffffffffffff   # kzg_rows_read out_overflow[1]: no cell overflowed
# kind -> (cell width in bytes, signed); name -> kind for the text client
COL_KINDS = {KZG_COL_BE32: (32, False), KZG_COL_U8: (1, False), KZG_COL_U16: (2, False), KZG_COL_U32: (4, False),
             KZG_COL_U64: (8, False), KZG_COL_I32: (4, True), KZG_COL_I64: (8, True)}
COL_DTYPES = {"fr": KZG_COL_BE32, "u8": KZG_COL_U8, "u16": KZG_COL_U16, "u32": KZG_COL_U32, "u64": KZG_COL_U64,
              "i32": KZG_COL_I32, "i64": KZG_COL_I64}
KZG_OK, KZG_E_ARG, KZG_E_SCALAR, KZG_E_POINT, KZG_E_HIP, KZG_E_NOMEM, KZG_E_BUSY, KZG_E_COMM = 0, -1, -2, -3, -4, -5, -6, -7
STATUS_NAMES = {0: "OK", -1: "E_ARG", -2: "E_SCALAR", -3: "E_POINT", -4: "E_HIP", -5: "E_NOMEM", -6: "E_BUSY", -7: "E_COMM"}
TIMING_NAMES = ["decode", "ntt", "digits", "scan", "scatter", "accumulate", "fixup", "tree", "final", "poly", "total", "collective"]

# every symbol include/kzg_mi355x.h (serving surface) and include/kzg_mi355x_test.h (test hooks) declare:
# name -> (restype, argtypes)
_P = ctypes.c_void_p
_B = ctypes.c_char_p
_U64, _U32, _I = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int


class QuotientGate(ctypes.Structure):
    """kzg_quotient_gate"""
    _fields_ = [("n_terms", _U32), ("coeffs_be32", _B), ("term_lens", ctypes.POINTER(_U32)), ("term_rows", ctypes.POINTER(_U32))]


class QuotientPerm(ctypes.Structure):
    """kzg_quotient_perm"""
    _fields_ = [("k", _U32), ("z_row", _U32), ("wire_rows", ctypes.POINTER(_U32)), ("sigma_rows", ctypes.POINTER(_U32)),
                ("shifts_be32", _B), ("beta_be32", _B), ("gamma_be32", _B), ("alpha_be32", _B)]


class QuotientTerms(ctypes.Structure):
    """kzg_quotient_terms"""
    _fields_ = [("n_terms", _U32), ("coeffs_be32", _B), ("term_lens", ctypes.POINTER(_U32)), ("term_rows", ctypes.POINTER(_U32)),
                ("term_rots", ctypes.POINTER(ctypes.c_int32))]


class QuotientLookup(ctypes.Structure):
    """kzg_quotient_lookup"""
    _fields_ = [("n_lookups", _U32), ("width", _U32), ("input_rows", ctypes.POINTER(_U32)), ("table_rows", ctypes.POINTER(_U32)),
                ("mult_row", _U32), ("sum_row", _U32), ("theta_be32", _B), ("beta_be32", _B), ("alpha_be32", _B)]


class QuotientActive(ctypes.Structure):
    """kzg_quotient_active"""
    _fields_ = [("active_row", _U32)]


class QuotientSelectors(ctypes.Structure):
    """kzg_quotient_selectors"""
    _fields_ = [("selector_rows", ctypes.POINTER(_U32))]


class ShuffleOpts(ctypes.Structure):
    """kzg_shuffle_opts"""
    _fields_ = [("n_sel_handles", _U32), ("sel_handles", ctypes.POINTER(_U64)), ("input_sel", ctypes.POINTER(_U32)),
                ("shuffle_sel", ctypes.POINTER(_U32)), ("usable", _U64), ("tail_be32", _B)]


class SortedOpts(ctypes.Structure):
    """kzg_sorted_opts"""
    _fields_ = [("usable", _U64), ("tail_be32", _B)]


class SigmaOpts(ctypes.Structure):
    """kzg_sigma_opts"""
    _fields_ = [("usable", _U64), ("free_label_be32", _B)]


class DeriveOp(ctypes.Structure):
    """kzg_derive_op"""
    _fields_ = [("kind", _U32), ("row", _U32), ("bits", _U32), ("count", _U32)]


class IntOp(ctypes.Structure):
    """kzg_int_op"""
    _fields_ = [("kind", _U32), ("width", _U32), ("a", _U32), ("b", _U32), ("imm", _U64), ("flags", _U32), ("count", _U32)]


class AluEntry(ctypes.Structure):
    """kzg_alu_entry"""
    _fields_ = [("kind", _U32), ("width", _U32), ("imm", _U64), ("flags", _U32), ("pad", _U32)]


class AluUnit(ctypes.Structure):
    """kzg_alu_unit"""
    _fields_ = [("op_row", _U32), ("a", _U32), ("b", _U32), ("count", _U32)]


class WideOp(ctypes.Structure):
    """kzg_wide_op"""
    _fields_ = [("kind", _U32), ("bits", _U32), ("limbs", _U32), ("count", _U32), ("flags", _U32), ("a", _U32), ("b", _U32),
                ("c", _U32), ("q", _U32), ("r", _U32), ("imm_be64", ctypes.c_uint8 * 64), ("m_be64", ctypes.c_uint8 * 64)]


class PoseidonParams(ctypes.Structure):
    """kzg_poseidon_params"""
    _fields_ = [("t", _U32), ("full", _U32), ("partial", _U32), ("rc_be32", ctypes.c_char_p), ("mds_be32", ctypes.c_char_p)]


class Poseidon2Params(ctypes.Structure):
    """kzg_poseidon2_params"""
    _fields_ = [("t", _U32), ("full", _U32), ("partial", _U32), ("rc_full_be32", ctypes.c_char_p),
                ("rc_partial_be32", ctypes.c_char_p), ("diag_be32", ctypes.c_char_p)]


class PoseidonUnit(ctypes.Structure):
    """kzg_poseidon_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("n_out", _U32), ("period", _U32), ("in_", _U32 * 8), ("out", _U32 * 8),
                ("expect", _U32 * 8), ("imm_be32", (ctypes.c_uint8 * 32) * 8)]


class PoseidonChainUnit(ctypes.Structure):
    """kzg_poseidon_chain_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("layout", _U32), ("period", _U32), ("start", _U32), ("pos", _U32),
                ("digest", _U32), ("expect", _U32), ("n_out", _U32), ("reserved", _U32), ("in_", _U32 * 8), ("out", _U32 * 16),
                ("imm_be32", (ctypes.c_uint8 * 32) * 8)]


class Sha256Unit(ctypes.Structure):
    """kzg_sha256_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("n_out", _U32), ("period", _U32), ("start", _U32), ("state", _U32 * 8),
                ("state_imm", _U32 * 8), ("msg", _U32 * 16), ("msg_imm", _U32 * 16), ("out", _U32 * 12), ("expect", _U32 * 8)]


class KeccakUnit(ctypes.Structure):
    """kzg_keccak_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("n_out", _U32), ("period", _U32), ("rate", _U32), ("start", _U32),
                ("imm", _U64 * 25), ("in_", _U32 * 25), ("out", _U32 * 16), ("expect", _U32 * 16)]


class EcCurve(ctypes.Structure):
    """kzg_ec_curve"""
    _fields_ = [("bits", _U32), ("limbs", _U32), ("p", _U64 * 4), ("a", _U64 * 4)]


class EcUnit(ctypes.Structure):
    """kzg_ec_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("cols", _U32), ("op", _U32), ("in_", _U32 * 4), ("expect", _U32 * 3),
                ("reserved", _U32), ("imm", _U64 * 4)]


class EdwardsCurve(ctypes.Structure):
    """kzg_edwards_curve"""
    _fields_ = [("a_be32", ctypes.c_uint8 * 32), ("d_be32", ctypes.c_uint8 * 32)]


class EdwardsUnit(ctypes.Structure):
    """kzg_edwards_unit"""
    _fields_ = [("mode", _U32), ("flags", _U32), ("cols", _U32), ("op", _U32), ("in_", _U32 * 4), ("expect", _U32 * 2),
                ("out_order", _U32 * 2), ("imm_be32", (ctypes.c_uint8 * 32) * 4)]


class Col(ctypes.Structure):
    """kzg_col"""
    _fields_ = [("data", ctypes.c_void_p), ("count", ctypes.c_uint64), ("kind", ctypes.c_uint32), ("fill_be32", ctypes.c_char_p)]


class DeriveOpts(ctypes.Structure):
    """kzg_derive_opts"""
    _fields_ = [("usable", _U64), ("tail_be32", _B)]


class Expr(ctypes.Structure):
    """kzg_expr"""
    _fields_ = [("terms", QuotientTerms), ("flags", _U32)]


class ExprOpts(ctypes.Structure):
    """kzg_expr_opts"""
    _fields_ = [("usable", _U64), ("tail_be32", _B)]


class Recurrence(ctypes.Structure):
    """kzg_recurrence"""
    _fields_ = [("mul", QuotientTerms), ("add", QuotientTerms), ("start_be32", _B)]


class RecurrenceOpts(ctypes.Structure):
    """kzg_recurrence_opts"""
    _fields_ = [("usable", _U64), ("tail_be32", _B)]


class QuotientLink(ctypes.Structure):
    """kzg_quotient_link"""
    _fields_ = [("prev_row", _U32), ("rot", ctypes.c_int32)]


SYMBOLS = {
    "kzg_create": (_I, [_I, ctypes.POINTER(_P)]),
    "kzg_destroy": (None, [_P]),
    "kzg_last_error": (ctypes.c_char_p, [_P]),
    "kzg_version": (ctypes.c_char_p, []),
    "kzg_runtime_info": (_I, [_P, ctypes.POINTER(ctypes.c_int32)]),
    "kzg_set_window": (_I, [_P, _I]),
    "kzg_get_window": (_I, [_P]),
    "kzg_get_window_layout": (_I, [_P, ctypes.POINTER(ctypes.c_int32), _I]),
    "kzg_load_srs": (_I, [_P, _B, _U64, _I, _I]),
    "kzg_load_srs_compressed": (_I, [_P, _B, _U64, _I, _I]),
    "kzg_load_srs_file": (_I, [_P, _B, _I, _I, _I]),
    "kzg_load_srs_file_slices": (_I, [_P, _B, _I, _I, _I, _U32, _U32]),
    "kzg_load_srs_file_range": (_I, [_P, _B, _I, _U64, _U64, _I]),
    "kzg_get_load_stats": (_I, [_P, ctypes.POINTER(ctypes.c_double)]),
    "kzg_set_srs_subgroup_check": (_I, [_P, _I]),
    "kzg_gen_srs": (_I, [_P, _B, _B, _U32, _I, _I]),
    "kzg_srs_points": (_U64, [_P]),
    "kzg_srs_read": (_I, [_P, _I, _U64, _U64, _B]),
    "kzg_srs_read_compressed": (_I, [_P, _I, _U64, _U64, _B]),
    "kzg_commit": (_I, [_P, _U32, _B, _U64, _I, _B]),
    "kzg_open": (_I, [_P, _U32, _B, _U64, _I, _B, _B, _B]),
    "kzg_commit_open": (_I, [_P, _U32, _B, _U64, _I, _B, _B, _B, _B]),
    "kzg_commit_open_batch": (_I, [_P, _U32, _U32, _B, _U64, _I, _B, _B, _B, _B, _B]),
    "kzg_commit_open_multi": (_I, [_P, _U32, _U32, _B, _U64, _I, _U32, _B, ctypes.POINTER(_U32), _B, _B, _B, _B]),
    "kzg_rows_commit": (_I, [_P, _U32, _U32, _B, _U64, _I, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_open": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(_U32), _B, _B, _B]),
    "kzg_rows_release": (_I, [_P, _U64]),
    "kzg_rows_commit_typed": (_I, [_P, _U32, _U32, ctypes.POINTER(Col), _U64, _I, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_read": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _U64, _U64, _U32, _I, ctypes.c_void_p, ctypes.POINTER(_U64)]),
    "kzg_rows_stats": (_I, [_P, ctypes.POINTER(_U64)]),
    "kzg_rows_eval": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(_U32), _B]),
    "kzg_rows_open_lincomb": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _U32, _B, _B, _B, _B]),
    "kzg_rows_commit_shplonk": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _U32, _B, ctypes.POINTER(_U32), _B, _B,
                                     ctypes.POINTER(_U64)]),
    "kzg_rows_commit_grand_product": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B, _B, _B, _B, _B,
                                           ctypes.POINTER(_U64)]),
    "kzg_rows_commit_shuffle": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _B, _B,
                                     ctypes.POINTER(ShuffleOpts), _B, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_sorted": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _U32, ctypes.POINTER(SortedOpts), _B,
                                    ctypes.POINTER(_U64)]),
    "kzg_rows_commit_int": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(IntOp), ctypes.POINTER(DeriveOpts), _B,
                                 ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_alu": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(AluEntry), _U32, ctypes.POINTER(AluUnit),
                                 ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                 ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_wide": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(WideOp), ctypes.POINTER(DeriveOpts), _B,
                                  ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                  ctypes.POINTER(_U64)]),
    "kzg_rows_commit_poseidon": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(PoseidonParams), _U32,
                                      ctypes.POINTER(PoseidonUnit), ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64),
                                      ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_poseidon2": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(Poseidon2Params), _U32,
                                       ctypes.POINTER(PoseidonUnit), ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64),
                                       ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_poseidon_chain": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(PoseidonParams), _U32,
                                            ctypes.POINTER(PoseidonChainUnit), ctypes.POINTER(DeriveOpts), _B]
                                       + [ctypes.POINTER(_U64)] * 7),
    "kzg_rows_commit_sha256": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Sha256Unit), ctypes.POINTER(DeriveOpts),
                                    _B] + [ctypes.POINTER(_U64)] * 7),
    "kzg_rows_commit_keccak": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(KeccakUnit), ctypes.POINTER(DeriveOpts),
                                    _B] + [ctypes.POINTER(_U64)] * 7),
    "kzg_rows_commit_ec": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(EcCurve), _U32, ctypes.POINTER(EcUnit),
                                ctypes.POINTER(DeriveOpts), _B] + [ctypes.POINTER(_U64)] * 10),
    "kzg_rows_commit_edwards": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(EdwardsCurve), _U32,
                                     ctypes.POINTER(EdwardsUnit), ctypes.POINTER(DeriveOpts), _B] + [ctypes.POINTER(_U64)] * 8),
    "kzg_rows_commit_derived": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(DeriveOp), ctypes.POINTER(DeriveOpts), _B,
                                     ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_expr": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Expr), ctypes.POINTER(ExprOpts), _B,
                                  ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_recurrence": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Recurrence),
                                        ctypes.POINTER(RecurrenceOpts), _B, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_fetch": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _U32,
                                   ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_sigma": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(SigmaOpts), _B, ctypes.POINTER(_U64),
                                   ctypes.POINTER(_U64)]),
    "kzg_rows_check_copies": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(SigmaOpts),
                                   ctypes.POINTER(_U64)]),
    "kzg_rows_commit_lookup_sum": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32, _U32, _B, _B, _B, _B,
                                        ctypes.POINTER(_U64)]),
    "kzg_rows_commit_multiplicities": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _B,
                                            ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_quotient": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientGate), ctypes.POINTER(QuotientPerm),
                                      _U32, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_quotient_ext": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms), ctypes.POINTER(QuotientPerm),
                                          ctypes.POINTER(QuotientLookup), _U32, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_grand_product_zk": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B, _B, _B, _U64, _B,
                                              _B, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_lookup_sum_zk": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32, _U32, _B, _B, _U64,
                                           _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_multiplicities_zk": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _U64, _B, _B,
                                               ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_lookup_sum_sel": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32,
                                            ctypes.POINTER(_U64), ctypes.POINTER(_U32), _U32, _U32, _B, _B, _U64, _B, _B, _B,
                                            ctypes.POINTER(_U64)]),
    "kzg_rows_commit_multiplicities_sel": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32,
                                                ctypes.POINTER(_U64), ctypes.POINTER(_U32), _U32, _U32, _U64, _B, _B,
                                                ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_rows_commit_quotient_sel": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms), ctypes.POINTER(QuotientPerm),
                                          ctypes.POINTER(QuotientLookup), ctypes.POINTER(QuotientSelectors),
                                          ctypes.POINTER(QuotientActive), _U32, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_quotient_part_sel": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms), ctypes.POINTER(QuotientPerm),
                                        ctypes.POINTER(QuotientLink), ctypes.POINTER(QuotientLookup),
                                        ctypes.POINTER(QuotientSelectors), ctypes.POINTER(QuotientActive), _U32, _B,
                                        ctypes.POINTER(_U64)]),
    "kzg_rows_commit_quotient_zk": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms), ctypes.POINTER(QuotientPerm),
                                         ctypes.POINTER(QuotientLookup), ctypes.POINTER(QuotientActive), _U32, _U32, _B,
                                         ctypes.POINTER(_U64)]),
    "kzg_rows_quotient_part": (_I, [_P, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms), ctypes.POINTER(QuotientPerm),
                                    ctypes.POINTER(QuotientLink), ctypes.POINTER(QuotientLookup), ctypes.POINTER(QuotientActive),
                                    _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_quotient_finish": (_I, [_P, _U64, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_rows_commit_grand_product_chain": (_I, [_P, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B, _B, _B, _U64,
                                                 _B, _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_commit_cached": (_I, [_P, _U32, _B, _U64, _I, _B, _B]),
    "kzg_open_cached": (_I, [_P, _U32, _B, _U64, _I, _B, _B, _B, _B]),
    "kzg_row_cache_stats": (_I, [_P, ctypes.POINTER(_U64)]),
    "kzg_msm": (_I, [_P, _B, _U64, _U64, _B]),
    "kzg_ntt": (_I, [_P, _B, _U64, _I]),
    "kzg_eval": (_I, [_P, _B, _U64, _B, _B]),
    "kzg_ntt_eval": (_I, [_P, _B, _U64, _I, _B, _B]),
    "kzg_vk_create": (_I, [_B, _B, _U32, ctypes.POINTER(_P)]),
    "kzg_vk_create_synthetic": (_I, [_B, _B, _U32, ctypes.POINTER(_P)]),
    "kzg_vk_destroy": (None, [_P]),
    "kzg_vk_export": (_I, [_P, _B, _U64]),
    "kzg_vk_verify": (_I, [_P, _U32, _B, _B, _B, _B, ctypes.POINTER(_I)]),
    "kzg_vk_verify_batch": (_I, [_P, _U32, ctypes.POINTER(_U32), _B, _B, _B, _B, _I, ctypes.POINTER(_I)]),
    "kzg_vk_verify_open_batch": (_I, [_P, _U32, _U32, _B, _B, _B, _B, _B, ctypes.POINTER(_I)]),
    "kzg_vk_verify_open_multi": (_I, [_P, _U32, _U32, _B, _U32, _B, ctypes.POINTER(_U32), _B, _B, _B, ctypes.POINTER(_I)]),
    "kzg_vk_verify_open_lincomb": (_I, [_P, _U32, _U32, _B, _U32, _B, _B, _B, _B, ctypes.POINTER(_I)]),
    "kzg_vk_verify_open_shplonk": (_I, [_P, _U32, _U32, _B, _U32, _B, ctypes.POINTER(_U32), _B, _B, _B, _B, _B,
                                        ctypes.POINTER(_I)]),
    "kzg_vk_pairing": (_I, [_B, _B, _B]),
    "kzg_msm_partial": (_I, [_P, _B, _U64, _U64, _B]),
    "kzg_g1_sum": (_I, [_P, _B, _U32, _B]),
    "kzg_msm_partial_resident_dev": (_I, [_P, _I, _U64, _U64, _P]),
    "kzg_g1_sum_dev": (_I, [_P, _P, _U32, _B]),
    "kzg_msm_sharded_begin": (_I, [_P, _I, _U64, _U64, _P, _P, ctypes.POINTER(_I)]),
    "kzg_msm_sharded_finish": (_I, [_P, _I, _P, _U32, _P, _B]),
    "kzg_comm_unique_id": (_I, [_B]),
    "kzg_comm_init": (_I, [_P, _B, _I, _I]),
    "kzg_comm_init_bounded": (_I, [_P, _B, _I, _I, _I]),
    "kzg_comm_destroy": (_I, [_P]),
    "kzg_comm_set_timeout": (_I, [_P, _I]),
    "kzg_comm_info": (_I, [_P, ctypes.POINTER(ctypes.c_int32)]),
    "kzg_comm_selftest": (_I, [_P]),
    "kzg_msm_sharded": (_I, [_P, _I, _U64, _U64, _B]),
    "kzg_test_comm_stall": (_I, [_P, _I]),
    "kzg_test_comm_stall_n": (_I, [_P, _I, _I]),
    "kzg_multi_create": (_I, [_I, ctypes.POINTER(_I), ctypes.POINTER(_P)]),
    "kzg_multi_destroy": (None, [_P]),
    "kzg_multi_last_error": (ctypes.c_char_p, [_P]),
    "kzg_multi_count": (_I, [_P]),
    "kzg_multi_ctx": (_P, [_P, _I]),
    "kzg_multi_device_of": (_I, [_P, _U32]),
    "kzg_multi_load_srs_file": (_I, [_P, _B, _I, _I, _I]),
    "kzg_multi_gen_srs": (_I, [_P, _B, _B, _I, _I]),
    "kzg_multi_load_srs_file_segments": (_I, [_P, _B, _I, _U64]),
    "kzg_multi_gen_srs_segments": (_I, [_P, _B, _B, _U64]),
    "kzg_multi_segment": (_I, [_P, _I, ctypes.POINTER(_U64)]),
    "kzg_multi_msm": (_I, [_P, _B, _U64, _U64, _B]),
    "kzg_multi_upload_fr": (_I, [_P, _I, _B, _U64, _U64]),
    "kzg_multi_msm_resident": (_I, [_P, _I, _B]),
    "kzg_multi_commit": (_I, [_P, _U32, _B, _U64, _I, _B]),
    "kzg_multi_open": (_I, [_P, _U32, _B, _U64, _I, _B, _B, _B]),
    "kzg_multi_commit_open": (_I, [_P, _U32, _B, _U64, _I, _B, _B, _B, _B]),
    "kzg_multi_commit_open_batch": (_I, [_P, _U32, _U32, _B, _U64, _I, _B, _B, _B, _B, _B]),
    "kzg_multi_commit_open_multi": (_I, [_P, _U32, _U32, _B, _U64, _I, _U32, _B, ctypes.POINTER(_U32), _B, _B, _B, _B]),
    "kzg_multi_rows_commit": (_I, [_P, _U32, _U32, _B, _U64, _I, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_open": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(_U32), _B, _B, _B]),
    "kzg_multi_rows_release": (_I, [_P, _U32, _U64]),
    "kzg_multi_rows_commit_typed": (_I, [_P, _U32, _U32, ctypes.POINTER(Col), _U64, _I, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_read": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _U64, _U64, _U32, _I, ctypes.c_void_p,
                                 ctypes.POINTER(_U64)]),
    "kzg_multi_rows_eval": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(_U32), _B]),
    "kzg_multi_rows_open_lincomb": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _U32, _B, _B, _B, _B]),
    "kzg_multi_rows_commit_shplonk": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _U32, _B, ctypes.POINTER(_U32), _B, _B,
                                           ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_grand_product": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B, _B, _B,
                                                 _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_shuffle": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _B, _B,
                                           ctypes.POINTER(ShuffleOpts), _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_sorted": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _U32, ctypes.POINTER(SortedOpts), _B,
                                          ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_int": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(IntOp),
                                       ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                       ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_alu": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(AluEntry), _U32,
                                       ctypes.POINTER(AluUnit), ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64),
                                       ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_wide": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(WideOp),
                                        ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                        ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_poseidon": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(PoseidonParams), _U32,
                                            ctypes.POINTER(PoseidonUnit), ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64),
                                            ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_poseidon2": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(Poseidon2Params), _U32,
                                             ctypes.POINTER(PoseidonUnit), ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64),
                                             ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_poseidon_chain": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(PoseidonParams), _U32,
                                                  ctypes.POINTER(PoseidonChainUnit), ctypes.POINTER(DeriveOpts), _B]
                                             + [ctypes.POINTER(_U64)] * 7),
    "kzg_multi_rows_commit_sha256": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Sha256Unit),
                                          ctypes.POINTER(DeriveOpts), _B] + [ctypes.POINTER(_U64)] * 7),
    "kzg_multi_rows_commit_keccak": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(KeccakUnit),
                                          ctypes.POINTER(DeriveOpts), _B] + [ctypes.POINTER(_U64)] * 7),
    "kzg_multi_rows_commit_ec": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(EcCurve), _U32, ctypes.POINTER(EcUnit),
                                      ctypes.POINTER(DeriveOpts), _B] + [ctypes.POINTER(_U64)] * 10),
    "kzg_multi_rows_commit_edwards": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(EdwardsCurve), _U32,
                                           ctypes.POINTER(EdwardsUnit), ctypes.POINTER(DeriveOpts), _B]
                                      + [ctypes.POINTER(_U64)] * 8),
    "kzg_multi_rows_commit_derived": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(DeriveOp),
                                           ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_expr": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Expr), ctypes.POINTER(ExprOpts), _B,
                                        ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_recurrence": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(Recurrence),
                                              ctypes.POINTER(RecurrenceOpts), _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_fetch": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32, _U32,
                                         ctypes.POINTER(DeriveOpts), _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                         ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_sigma": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, _B, ctypes.POINTER(SigmaOpts), _B,
                                         ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_check_copies": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32,
                                         ctypes.POINTER(SigmaOpts), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_lookup_sum": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32, _U32, _B,
                                              _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_multiplicities": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32,
                                                  _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_quotient": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientGate),
                                            ctypes.POINTER(QuotientPerm), _U32, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_quotient_ext": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms),
                                                ctypes.POINTER(QuotientPerm), ctypes.POINTER(QuotientLookup), _U32, _U32, _B,
                                                ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_grand_product_zk": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B, _B,
                                                    _B, _U64, _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_lookup_sum_zk": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32, _U32,
                                                 _B, _B, _U64, _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_multiplicities_zk": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _U32,
                                                     _U64, _B, _B, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_lookup_sum_sel": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U64, _U32,
                                                  ctypes.POINTER(_U64), ctypes.POINTER(_U32), _U32, _U32, _B, _B, _U64, _B, _B, _B,
                                                  ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_multiplicities_sel": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32,
                                                      ctypes.POINTER(_U64), ctypes.POINTER(_U32), _U32, _U32, _U64, _B, _B,
                                                      ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_quotient_sel": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms),
                                                ctypes.POINTER(QuotientPerm), ctypes.POINTER(QuotientLookup),
                                                ctypes.POINTER(QuotientSelectors), ctypes.POINTER(QuotientActive), _U32, _U32, _B,
                                                ctypes.POINTER(_U64)]),
    "kzg_multi_rows_quotient_part_sel": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms),
                                              ctypes.POINTER(QuotientPerm), ctypes.POINTER(QuotientLink),
                                              ctypes.POINTER(QuotientLookup), ctypes.POINTER(QuotientSelectors),
                                              ctypes.POINTER(QuotientActive), _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_quotient_zk": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms),
                                               ctypes.POINTER(QuotientPerm), ctypes.POINTER(QuotientLookup),
                                               ctypes.POINTER(QuotientActive), _U32, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_quotient_part": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(QuotientTerms),
                                          ctypes.POINTER(QuotientPerm), ctypes.POINTER(QuotientLink),
                                          ctypes.POINTER(QuotientLookup), ctypes.POINTER(QuotientActive), _U32, _B,
                                          ctypes.POINTER(_U64)]),
    "kzg_multi_rows_quotient_finish": (_I, [_P, _U32, _U64, _U32, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_rows_commit_grand_product_chain": (_I, [_P, _U32, _U32, ctypes.POINTER(_U64), _U32, ctypes.POINTER(_U64), _U32, _B,
                                                       _B, _B, _U64, _B, _B, _B, _B, ctypes.POINTER(_U64)]),
    "kzg_multi_commit_open_rows": (_I, [_P, _U32, ctypes.POINTER(_U32), _B, _U64, _I, _B, _B, _B, _B, ctypes.POINTER(_I)]),
    "kzg_upload_fr": (_I, [_P, _I, _B, _U64, _I]),
    "kzg_msm_resident": (_I, [_P, _I, _U64, _U64, _B]),
    "kzg_msm_partial_resident": (_I, [_P, _I, _U64, _U64, _B]),
    "kzg_msm_submit": (_I, [_P, _I, _U64, _U64, _I, ctypes.POINTER(_I)]),
    "kzg_msm_wait": (_I, [_P, _I, _B]),
    "kzg_msm_cancel": (_I, [_P, _I]),
    "kzg_commit_open_resident": (_I, [_P, _U32, _I, _U64, _I, _B, _B, _B, _B]),
    "kzg_ntt_resident": (_I, [_P, _I, _U64, _I]),
    "kzg_staging_acquire": (_I, [_P, _U64, ctypes.POINTER(_P), ctypes.POINTER(_I)]),
    "kzg_staging_release": (_I, [_P, _I]),
    "kzg_staging_flush": (_I, [_P, _I, _U64, _U64]),
    "kzg_set_host_finish": (_I, [_P, _I]),
    "kzg_host_xyzz_to_c48": (_I, [_P, _B]),
    "kzg_host_xyzz_pair_to_c48": (_I, [_P, _P, _B, _B]),
    "kzg_host_xyzz_to_partial192": (_I, [_P, _B]),
    "kzg_g1_sum_compressed": (_I, [_P, _B, _U32, _B]),
    "kzg_set_profiling": (_I, [_P, _I]),
    "kzg_get_timings": (_I, [_P, ctypes.POINTER(ctypes.c_float), _I]),
    "kzg_msm_plan": (_I, [_P, _U64, ctypes.POINTER(ctypes.c_int32)]),
    "kzg_calibrate": (_I, [_P, _I, ctypes.POINTER(ctypes.c_double)]),
    "kzg_b64_decode_fr": (_I, [_B, _U64, _B]),
    "kzg_b64_encode_fr": (_I, [_B, _U64, _B]),
    "kzg_test_field": (_I, [_P, _I, _I, _B, _B, _B, _U64]),
    "kzg_test_g1": (_I, [_P, _I, _B, _B, _B, _U64]),
    "kzg_test_fp_raw": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _U64]),
    "kzg_test_g1_raw": (_I, [_P, _I, _P, _P, _B, _U64]),
    "kzg_test_ntt_plan_of": (_I, [_I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "kzg_test_ntt_run": (_I, [_P, _P, _I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "kzg_test_msm_passes": (_I, [_I, _I, _U32, _U32, ctypes.POINTER(_U32), ctypes.POINTER(_I)]),
    "kzg_test_poly_plan_of": (_I, [_U64, _I, ctypes.c_int64, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I),
                                   ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "kzg_test_poly_run": (_I, [_P, _I, _I, ctypes.c_int64, _I, _I, _P, _U64, _U32, _I, _P, _P, _U32, _P, _P, _U32, _P, _P]),
    "kzg_test_join": (_I, [_P, _I, _I, _P, _P, _P, _U64, _U64, _U32, _U32, _I, _U32, _P, _P, _P, _P, ctypes.POINTER(_U64),
                           ctypes.POINTER(_U64), ctypes.POINTER(_U32)]),
    "kzg_test_join_counts": (_I, [_P, _P, _U64, _P]),
}

# the plan hooks of the recurrence scan (include/kzg_mi355x_recur_test.h, which kzg_mi355x_test.h includes): bound like SYMBOLS
RECUR_HOOKS = {
    "kzg_test_recur_plan_of": (_I, [_U64, _I, ctypes.c_int64, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_U64),
                                    ctypes.POINTER(_U64)]),
    "kzg_test_recur_run": (_I, [_P, _I, ctypes.c_int64, _P, _P, _P, _U64, _P, _P]),
}

# the plan hooks of the product and the additive scan (include/kzg_mi355x_scan_test.h, likewise): bound like SYMBOLS
SCAN_HOOKS = {
    "kzg_test_scan_plan_of": (_I, [_U64, _I, ctypes.c_int64, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_U64),
                                   ctypes.POINTER(_U64)]),
    "kzg_test_scan_run": (_I, [_P, _I, _I, ctypes.c_int64, _P, _P, _P, _U64, _P, _P, ctypes.POINTER(_U32)]),
}

_lib = None


class KzgError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"kzg_mi355x {STATUS_NAMES.get(code, code)}: {message}")
        self.code = code


def open_masks(opened, k: int):
    """The multi-point opening's row masks (bit j = row j) from opened[p], point p's rows as a strictly increasing list of
    indices in [0, k); a (ctypes uint32 array, number of evaluations).  KzgError(KZG_E_ARG) for anything else."""
    m = len(opened)
    if m == 0 or m > KZG_MAX_OPEN_POINTS:
        raise KzgError(KZG_E_ARG, f"multi-point opening: {m} points, expected 1 .. {KZG_MAX_OPEN_POINTS}")
    masks = (ctypes.c_uint32 * m)()
    for p, rows in enumerate(opened):
        rows = [int(j) for j in rows]
        if not rows or any(b <= a for a, b in zip(rows, rows[1:])) or rows[0] < 0 or rows[-1] >= k:
            raise KzgError(KZG_E_ARG, f"multi-point opening: point {p} opens {rows}, expected increasing rows in [0, {k})")
        masks[p] = sum(1 << j for j in rows)
    return masks, sum(len(r) for r in opened)


def shplonk_masks(opened, k: int):
    """The SHPLONK row masks (bit j = row j) from opened[p], the rows opened at point p as a strictly increasing list of
    indices in [0, k) (it may be empty: the point then only enters Z_P); a (ctypes uint32 array, number of evaluations).
    KzgError(KZG_E_ARG) for anything else."""
    m = len(opened)
    if m == 0 or m > KZG_MAX_SHPLONK_POINTS:
        raise KzgError(KZG_E_ARG, f"shplonk: {m} points, expected 1 .. {KZG_MAX_SHPLONK_POINTS}")
    masks = (ctypes.c_uint32 * m)()
    for p, rows in enumerate(opened):
        rows = [int(j) for j in rows]
        if any(b <= a for a, b in zip(rows, rows[1:])) or (rows and (rows[0] < 0 or rows[-1] >= k)):
            raise KzgError(KZG_E_ARG, f"shplonk: point {p} opens {rows}, expected increasing rows in [0, {k})")
        masks[p] = sum(1 << j for j in rows)
    return masks, sum(len(r) for r in opened)


def lib_available() -> bool:
    return os.path.exists(LIB_PATH)


def load() -> ctypes.CDLL:
    """Loads the HIP library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m zkp_subnet_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
            )
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(RECUR_HOOKS.items()) + list(SCAN_HOOKS.items()):
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
