"""Thin object wrapper over the C-ABI: one HipEngine = one kzg_ctx = one MI355X.

All arguments and results are bytes in the wire layouts of include/kzg_mi355x.h (Fr 32 B big-endian, G1 affine
96 B / compressed 48 B).  This is the object `Client` drives; tests inject an oracle-backed stand-in with the same
methods to exercise the host logic on machines without a GPU."""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native
from ._native import KzgError
from .verifier import shplonk_finish_coeffs

R_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _root_of_unity(n: int) -> int:
    return pow(7, (R_MODULUS - 1) // n, R_MODULUS)


def lagrange_factor(i: int, machines_scale: int, tau_y: int) -> int:
    """L_i(tau_y) over the 2^machines_scale-point Y domain: the per-worker factor of the Pianist SRS slice
    U_{i,j} = tau_x^j L_i(tau_y) G.  Setup-time host arithmetic only."""
    m = 1 << machines_scale
    if m == 1:
        return 1
    wi = pow(_root_of_unity(m), i, R_MODULUS)
    if (tau_y - wi) % R_MODULUS == 0:
        return 1
    num = (pow(tau_y, m, R_MODULUS) - 1) % R_MODULUS
    inv = lambda v: pow(v % R_MODULUS, R_MODULUS - 2, R_MODULUS)  # noqa: E731
    return wi * inv(m) % R_MODULUS * num % R_MODULUS * inv(tau_y - wi) % R_MODULUS


def shuffle_quotient_terms(z_row: int, input_rows: Sequence[int], shuffle_rows: Sequence[int], n_groups: int, width: int,
                           theta_be32: bytes, gamma_be32: bytes, coeff_be32: bytes, active_row: Optional[int] = None,
                           input_sel: Optional[Sequence[Optional[int]]] = None,
                           shuffle_sel: Optional[Sequence[Optional[int]]] = None,
                           ext_log: int = 2) -> List[Tuple[bytes, List[Tuple[int, int]]]]:
    """The relation that makes commit_shuffle's z an argument, as gate terms for commit_quotient_ext / _zk / quotient_part:
        coeff * A * [ z(wX) prod_g df_g(X)  -  z(X) prod_g nf_g(X) ]
    multiplied out over the groups into (32-byte coefficient, [(row, rot), ..]) terms.  Every argument names a row of the
    quotient call's concatenation: z, the n_groups * width input and shuffle rows (group-major), the optional active column A
    and, per group, None or the selector row of that side (input_sel / shuffle_sel, None: no selector at all); theta and gamma
    are those z was built with, coeff the caller's power of alpha.  Terms with the same factors are added up and nothing
    else is merged.  Raises CodecError when the expansion needs more than KZG_MAX_GATE_TERMS terms or a term more than
    2^ext_log + 1 factors: such a relation goes through quotient_part in slices of this list, or needs a larger ext_log.
    "z = 1 at row 0" and, under blinding, "z = 1 at row u" are not written here: they stay the ordinary gate terms (z - 1) L_0
    and (z - 1) L_u over a caller row L_0 / L_u, as for the permutation.  Pure host arithmetic on a few scalars."""
    from . import codec

    G, w = int(n_groups), int(width)
    if G < 1 or w < 1 or len(input_rows) != G * w or len(shuffle_rows) != G * w:
        raise codec.CodecError(f"shuffle_quotient_terms: n_groups, width >= 1 and n_groups * width = {G * w} input and shuffle "
                               f"rows each, not {len(input_rows)} and {len(shuffle_rows)}")
    sels = [[None] * G if s is None else list(s) for s in (input_sel, shuffle_sel)]
    if any(len(s) != G for s in sels):
        raise codec.CodecError(f"shuffle_quotient_terms: input_sel and shuffle_sel hold one entry per group ({G}) or are None")
    if any(len(x) != 32 or int.from_bytes(x, "big") >= R_MODULUS for x in (theta_be32, gamma_be32, coeff_be32)):
        raise codec.CodecError("shuffle_quotient_terms: theta, gamma and coeff must be canonical scalars (< r) of 32 bytes")
    theta, gamma, coeff = (int.from_bytes(x, "big") for x in (theta_be32, gamma_be32, coeff_be32))

    def factor(rows, q):   # gamma + sum_c theta^c row_c, or 1 + q (gamma - 1) + sum_c theta^c q row_c, as {factors: coefficient}
        head = [] if q is None else [(int(q), 0)]
        mono = [((), 1), (tuple(head), gamma - 1)] if head else [((), gamma)]
        return mono + [(tuple(head + [(int(rows[c]), 0)]), pow(theta, c, R_MODULUS)) for c in range(w)]

    out: Dict[tuple, int] = {}
    front = [] if active_row is None else [(int(active_row), 0)]
    for side, rows, rot, sign in ((1, shuffle_rows, 1, 1), (0, input_rows, 0, -1)):
        prod = [(tuple(front + [(int(z_row), rot)]), sign * coeff % R_MODULUS)]
        for g in range(G):
            f = factor(rows[g * w:(g + 1) * w], sels[side][g])
            prod = [(fa + fb, ca * cb % R_MODULUS) for fa, ca in prod for fb, cb in f]
        for fs, c in prod:
            key = tuple(sorted(fs))
            out[key] = (out.get(key, 0) + c) % R_MODULUS
    E = 1 << int(ext_log)
    if len(out) > _native.KZG_MAX_GATE_TERMS:
        raise codec.CodecError(f"shuffle_quotient_terms: the relation expands into {len(out)} terms, more than "
                               f"KZG_MAX_GATE_TERMS = {_native.KZG_MAX_GATE_TERMS}")
    deepest = max(len(fs) for fs in out)
    if deepest > E + 1:
        raise codec.CodecError(f"shuffle_quotient_terms: a term has {deepest} factors, more than 2^ext_log + 1 = {E + 1}")
    return [(c.to_bytes(32, "big"), list(fs)) for fs, c in out.items()]


_TYPED_FORMATS = {("B", 1): _native.KZG_COL_U8, ("H", 2): _native.KZG_COL_U16, ("I", 4): _native.KZG_COL_U32,
                  ("L", 8): _native.KZG_COL_U64, ("Q", 8): _native.KZG_COL_U64, ("i", 4): _native.KZG_COL_I32,
                  ("l", 8): _native.KZG_COL_I64, ("q", 8): _native.KZG_COL_I64}


def typed_column(col, what: str = "commit_rows_typed"):
    """One column of commit_rows_typed as (kind, cells, memoryview of its bytes, fill or None).  `col` is a buffer or a
    (buffer, fill_be32_or_None) pair.  bytes / bytearray of 32 * cells are 32-byte big-endian scalars (KZG_COL_BE32); any other
    object with the buffer protocol (numpy arrays, array.array, memoryviews) must be one-dimensional and C-contiguous with the
    native format B, H, I, L / Q, i or l / q at item size 1, 2, 4, 8, 4, 8.  Nothing is copied here; commit_rows_typed hands the
    library the buffer's own memory when it is writable or a whole bytes object, and one copy of a read-only view otherwise.
    Raises KzgError(KZG_E_ARG)."""
    bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
    buf, fill = col if isinstance(col, tuple) and len(col) == 2 else (col, None)
    if fill is not None and (not isinstance(fill, (bytes, bytearray)) or len(fill) != 32):
        raise bad("a fill is None or 32 big-endian bytes")
    if isinstance(buf, (bytes, bytearray)):
        if len(buf) % 32:
            raise bad("a bytes column holds 32 bytes per cell")
        return _native.KZG_COL_BE32, len(buf) // 32, memoryview(buf), fill
    try:
        mv = memoryview(buf)
    except TypeError:
        raise bad(f"a column is bytes or an object with the buffer protocol, not {type(buf).__name__}") from None
    if mv.ndim != 1 or not mv.c_contiguous:
        raise bad("a column must be one-dimensional and C-contiguous")
    fmt = mv.format[1:] if mv.format[:1] in "@=<" and len(mv.format) > 1 else mv.format
    kind = _TYPED_FORMATS.get((fmt, mv.itemsize))
    if kind is None:
        raise bad(f"unsupported buffer format {mv.format!r} with item size {mv.itemsize}: expected B, H, I, L/Q, i or l/q "
                  f"(u8, u16, u32, u64, i32, i64)")
    return kind, mv.shape[0], mv, fill


_R_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
_is_u = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < top   # noqa: E731
_ZERO32 = bytes(32)
_pad = lambda xs, k, fill=0: list(xs) + [fill] * (k - len(xs))   # noqa: E731


class _UnitSpec:
    """The field parsers of one call of a unit encoder (poseidon_call .. edwards_call): a call is a list of units, each a
    mapping with a mode; a unit's slots are row indices or ("imm", value), it has an out / cols list and an optional expect,
    and the call may name and commit at most KZG_MAX_BATCH_OPEN rows.  The words that differ between the builders are
    arguments; `seen` collects the distinct input rows.  Every refusal is KzgError(KZG_E_ARG, "<what>: <chip>: <why>")."""

    def __init__(self, what: str, chip: str):
        self.head, self.seen = f"{what}: {chip}: ", set()

    def bad(self, why) -> KzgError:
        """why: the words, or a function that makes them -- words that need formatting are made on refusal only"""
        return KzgError(_native.KZG_E_ARG, self.head + (why if isinstance(why, str) else why()))

    def scalar(self, v, name: str) -> bytes:
        """a canonical scalar given as an int, a decimal or 0x string, or 32 big-endian bytes, as 32 bytes"""
        if isinstance(v, (bytes, bytearray)):
            if len(v) != 32:
                raise self.bad(f"{name} given as bytes must be of 32 bytes")
            v = int.from_bytes(v, "big")
        elif isinstance(v, str):
            try:
                v = int(v, 0)
            except ValueError:
                raise self.bad(f"{name} must be an integer, a decimal or 0x string, or 32 bytes") from None
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise self.bad(f"{name} must be a non-negative integer")
        if v >= _R_MODULUS:
            raise self.bad(f"{name} must be a canonical scalar (< r)")
        return v.to_bytes(32, "big")

    def units(self, units, top: int) -> list:
        units = list(units) if isinstance(units, (list, tuple)) else None
        if not units or len(units) > top:
            raise self.bad(f"units must be a list of 1 .. {top} entries (n_units)")
        return units

    def mode(self, un, keys: dict, expect_why: Optional[str] = None, foreign: bool = False) -> str:
        """the mode of the unit `un`, whose fields must be among keys[mode].  expect_why: the refusal of an expect the mode
        does not take; foreign: a field of another mode has a refusal of its own"""
        if not isinstance(un, dict) or "mode" not in un:
            raise self.bad("a unit is a mapping with mode and the fields of its mode")
        mode = un["mode"]
        if not isinstance(mode, str) or mode not in keys:
            raise self.bad(f"unknown mode {mode!r} (one of " + ", ".join('"%s"' % m for m in keys) + ")")
        extra = set(un) - set(keys[mode])
        if extra:
            name = sorted(extra)[0]
            if expect_why and "expect" in extra:
                raise self.bad(expect_why)
            if foreign and any(name in ks for ks in keys.values()):
                raise self.bad(f"a field the mode does not take: {name!r} does not belong to a {mode} unit")
            raise self.bad(f"unknown field {name!r} (the fields of a {mode} unit are {', '.join(keys[mode])})")
        return mode

    def row(self, v, why, top: int = 0xffffffff) -> int:
        """a row index below top (why: its refusal)"""
        if not _is_u(v, top):
            raise self.bad(why)
        self.seen.add(v)
        return v

    def slot(self, v, name: str, imm_bits: int = 0, top: int = 0xffffffff) -> tuple:
        """a row index or ("imm", value): (the row, a zero) or (top, the immediate) -- an integer below 2^imm_bits, or for
        imm_bits = 0 a canonical scalar as 32 bytes"""
        if isinstance(v, (list, tuple)):
            if len(v) != 2 or v[0] != "imm":
                raise self.bad('an immediate is ("imm", value)')
            if not imm_bits:
                return top, self.scalar(v[1], "an immediate")
            if not _is_u(v[1], 1 << imm_bits):
                raise self.bad(f"an immediate must be an integer below 2^{imm_bits}")
            return top, v[1]
        if not _is_u(v, top):
            raise self.bad(f'{name} must be a row index, an integer in [0, 2^32 - 1), or ("imm", value)')
        self.seen.add(v)
        return v, (0 if imm_bits else _ZERO32)

    def slots(self, v, count: int, why: str, name: str, imm_bits: int = 0) -> tuple:
        """a list of `count` slots (why: the refusal of anything else): (the rows, the immediates)"""
        if not isinstance(v, (list, tuple)) or len(v) != count:
            raise self.bad(why)
        rows, imms, see, zero = [], [], self.seen.add, (0 if imm_bits else _ZERO32)
        for s in v:
            if type(s) is int and 0 <= s < 0xffffffff:   # (the plain case without a call: it is met per slot of every call)
                see(s)
                imm = zero
            else:
                s, imm = self.slot(s, name, imm_bits)
            rows.append(s)
            imms.append(imm)
        return rows, imms

    def period(self, v, lo: int, why: str) -> int:
        if not _is_u(v, 1 << 32) or v < lo:
            raise self.bad(why)
        return v

    def indices(self, v, most: int, top: int, why: str, why_index: str, why_repeated: str) -> list:
        """an out list: 1 .. most distinct indices below top"""
        if not isinstance(v, (list, tuple)) or not 1 <= len(v) <= most:
            raise self.bad(why)
        if any(not _is_u(j, top) for j in v):
            raise self.bad(why_index)
        if len(set(v)) != len(v):
            raise self.bad(why_repeated)
        return list(v)

    def expects(self, v, n: int) -> list:
        """an expect list: one row per entry of out"""
        if not isinstance(v, (list, tuple)) or len(v) != n:
            raise self.bad("expect must hold one row per entry of out")
        if any(not _is_u(j, 0xffffffff) for j in v):
            raise self.bad("an entry of expect must be a row index, an integer in [0, 2^32 - 1)")
        self.seen.update(v)
        return list(v)

    def names(self, v, allowed, why, kind: str = "column name", unit: str = "", top: Optional[int] = None) -> list:
        """a list of 1 .. top (None: any number of) distinct names among `allowed`, as their indices; unit: the mode whose
        names they are, where the refusal says so"""
        if not isinstance(v, (list, tuple)) or not v or (top is not None and len(v) > top):
            raise self.bad(why)
        for name in v:
            if name not in allowed:
                raise self.bad(f"unknown {kind} {name!r} (the names{unit and f' of a {unit} unit'} are {', '.join(allowed)})")
        if len(set(v)) != len(v):
            raise self.bad(f"a {kind} is repeated")
        return [allowed.index(name) for name in v]

    def out_or_expect(self, un) -> bool:
        """a unit commits (out) or is a check (expect): whether it is a check"""
        has_out, has_exp = un.get("out") is not None, un.get("expect") is not None
        if has_out and has_exp:
            raise self.bad("out together with expect: a unit commits, or it is a check")
        if not has_out and not has_exp:
            raise self.bad("a unit needs out, or expect for a check")
        return has_exp

    def caps(self, n_out: int) -> None:
        """the two closing caps of a call"""
        top = _native.KZG_MAX_BATCH_OPEN
        if len(self.seen) > top:
            raise self.bad(f"the units read {len(self.seen)} distinct input rows, at most {top} fit one call")
        if n_out > top:
            raise self.bad(f"n_out: the units give {n_out} output rows, at most {top} fit one call")


class HipEngine:
    # rows from this length up are decoded and uploaded tile by tile (see _Staged); KZG_STREAM_MIN_LOG moves the threshold
    STREAM_MIN = 1 << int(os.environ.get("KZG_STREAM_MIN_LOG", "19"))
    STREAM_TILE = 1 << int(os.environ.get("KZG_STREAM_TILE_LOG", "18"))   # 2^18 elements: the decode pool's full thread count

    def __init__(self, device: int = 0, window: int = 0):
        self._lib = _native.load()
        h = ctypes.c_void_p()
        rc = self._lib.kzg_create(device, ctypes.byref(h))
        if rc != 0:
            raise KzgError(rc, "kzg_create failed: no usable gfx950 device (this build has no CPU fallback)")
        self._h = h
        self.device = device
        self.scale = self.machines_scale = 0
        self.verifier = None          # host-side pairing verifier (zkp_subnet_amd.verifier.Verifier)
        self._set_len: Dict[int, Tuple[int, int]] = {}   # handle -> (worker, row length) of the live sets made through RowSet
        self._set_rows: Dict[int, int] = {}   # handle -> rows of those sets (commit_fetch: the table's width sizes its output)
        if window:
            self._chk(self._lib.kzg_set_window(self._h, window))

    # ------------------------------------------------------------------ plumbing
    def _chk(self, rc: int) -> None:
        if rc != 0:
            raise KzgError(rc, self._lib.kzg_last_error(self._h).decode(errors="replace"))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.kzg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def runtime_info(self) -> Dict[str, int]:
        """What kzg_create measured: lanes of the context, how many of them really run concurrently (hardware queues),
        whether a HIP runtime was already live when the library was loaded, GPU_MAX_HW_QUEUES as seen (0 = unset)."""
        arr = (ctypes.c_int32 * 4)()
        self._chk(self._lib.kzg_runtime_info(self._h, arr))
        return {"lanes": arr[0], "lanes_concurrent": arr[1], "hip_live_at_load": bool(arr[2]), "hw_queues_env": arr[3]}

    @property
    def window(self) -> int:
        return self._lib.kzg_get_window(self._h)

    @property
    def window_offsets(self) -> List[int]:
        """Bit offset of every Pippenger window plus the closing 256 (table w holds 2^offset[w] * P)."""
        arr = (ctypes.c_int32 * 70)()
        nwin = self._lib.kzg_get_window_layout(self._h, arr, 70)
        if nwin < 0:
            raise KzgError(nwin, "no window layout yet (load an SRS first)")
        return list(arr[: nwin + 1])

    @property
    def srs_points(self) -> int:
        return self._lib.kzg_srs_points(self._h)

    @property
    def slice_len(self) -> int:
        return 1 << (self.scale - self.machines_scale)

    # ------------------------------------------------------------------ SRS
    def load_srs(self, points: bytes, scale: int, machines_scale: int, compressed: bool = False) -> None:
        """`points`: 96-byte uncompressed affine records, or 48-byte ZCash-compressed ones (`compressed=True`)."""
        if compressed:
            self._chk(self._lib.kzg_load_srs_compressed(self._h, points, len(points) // 48, scale, machines_scale))
        else:
            self._chk(self._lib.kzg_load_srs(self._h, points, len(points) // 96, scale, machines_scale))
        self.scale, self.machines_scale = scale, machines_scale
        self.verifier = None

    def load_srs_file(self, path: str, scale: int, machines_scale: int, compressed: bool = False) -> None:
        """The setup FILE the reference prover is started with (base/miner.py:75-84): read by the library with
        pread(2) straight into two pinned tiles (host read, upload and GPU decode overlap), never into Python memory."""
        self._chk(self._lib.kzg_load_srs_file(self._h, os.fsencode(path), int(compressed), scale, machines_scale))
        self.scale, self.machines_scale = scale, machines_scale
        self.verifier = None

    def load_srs_file_slices(self, path: str, scale: int, machines_scale: int, first_slice: int, slice_stride: int,
                             compressed: bool = False) -> None:
        """Only the slices one device of a multi-GPU host serves: resident slice k = file slice first_slice + k * stride
        (worker i = g mod G on device g).  pread touches just those byte ranges (kzg_load_srs_file_slices)."""
        self._chk(self._lib.kzg_load_srs_file_slices(self._h, os.fsencode(path), int(compressed), scale, machines_scale,
                                                     first_slice, slice_stride))
        self.scale, self.machines_scale = scale, machines_scale
        self.verifier = None

    def load_srs_file_range(self, path: str, first_point: int, n_points: int, compressed: bool = False) -> None:
        """One contiguous segment of a flat SRS file as a single resident slice (kzg_load_srs_file_range)."""
        scale = max(0, (n_points - 1).bit_length())
        self._chk(self._lib.kzg_load_srs_file_range(self._h, os.fsencode(path), int(compressed), first_point, n_points, scale))
        self.scale, self.machines_scale = scale, 0
        self.verifier = None

    def set_srs_subgroup_check(self, enable: bool) -> None:
        """Loaders test every SRS point for membership in G1 (default on).  False skips it for the NEXT load only (a file
        of established provenance); the library arms the check again after that load."""
        self._chk(self._lib.kzg_set_srs_subgroup_check(self._h, int(enable)))

    def load_stats(self) -> Dict[str, float]:
        """Seconds of the last successful SRS load: host copies, waits for upload + decode, window tables, total."""
        arr = (ctypes.c_double * 4)()
        self._chk(self._lib.kzg_get_load_stats(self._h, arr))
        return {"host_copy_s": arr[0], "gpu_wait_s": arr[1], "tables_s": arr[2], "total_s": arr[3]}

    def set_verifier_key(self, tau_g2_be192: bytes, li_g1_be96: bytes) -> None:
        """Verification key of a loaded SRS: [tau_x]_2 (uncompressed G2, 192 B) and [L_i(tau_y)]_1 per resident slice."""
        from .verifier import Verifier

        self.verifier = Verifier.from_points(tau_g2_be192, li_g1_be96)

    def gen_srs(self, tau_x: int, tau_y: int, scale: int, machines_scale: int,
                workers: Optional[Sequence[int]] = None, factors: Optional[Sequence[int]] = None) -> None:
        """Synthetic tau-derived SRS for the listed worker indices (default: all 2^machines_scale), slice k of
        the resident SRS = worker workers[k].  NOTE: resident slice index == position in `workers`.
        `factors` overrides the per-slice factor s0_k (slice k, point j = [s0_k tau_x^j] G): bench.py uses it to
        generate one SRS *segment* per rank (s0 = tau^(rank * n_local))."""
        if factors is not None:
            s0 = b"".join((f % R_MODULUS).to_bytes(32, "big") for f in factors)
        else:
            if workers is None:
                workers = range(1 << machines_scale)
            s0 = b"".join(lagrange_factor(i, machines_scale, tau_y).to_bytes(32, "big") for i in workers)
        self._chk(self._lib.kzg_gen_srs(self._h, (tau_x % R_MODULUS).to_bytes(32, "big"), s0, len(s0) // 32, scale,
                                        machines_scale))
        self.scale, self.machines_scale = scale, machines_scale
        from .verifier import Verifier

        self.verifier = Verifier.synthetic(tau_x % R_MODULUS, [int.from_bytes(s0[i:i + 32], "big")
                                                               for i in range(0, len(s0), 32)])

    def verify(self, i: int, proof48: bytes, alpha32: bytes, eval32: bytes, commitment48: bytes) -> bool:
        """Pairing check of one opening against resident slice i (host-side; reference neurons/validator.py:77-86)."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify(i, proof48, alpha32, eval32, commitment48)

    def verify_batch(self, indices: Sequence[int], proofs48: Sequence[bytes], alpha32: bytes, evals32: Sequence[bytes],
                     commitments48: Sequence[bytes], threads: int = 16) -> bool:
        """All rows of a validator step (common alpha) in one pairing check; True only if every row is valid."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify_batch(indices, proofs48, alpha32, evals32, commitments48, threads)

    def verify_open_batch(self, i: int, commitments48: Sequence[bytes], evals32: Sequence[bytes], alpha32: bytes,
                          gamma32: bytes, proof48: bytes) -> bool:
        """Pairing check of one batched opening (commit_open_batch) against resident slice i."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify_open_batch(i, commitments48, evals32, alpha32, gamma32, proof48)

    def verify_open_multi(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                          opened: Sequence[Sequence[int]], gammas32: Sequence[bytes], evals32: Sequence[Sequence[bytes]],
                          proofs48: Sequence[bytes]) -> bool:
        """Pairing check of one multi-point opening (commit_open_multi) against resident slice i."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify_open_multi(i, commitments48, points32, opened, gammas32, evals32, proofs48)

    def srs_read(self, first: int, count: int, window: int = 0, compressed: bool = False) -> bytes:
        out = ctypes.create_string_buffer((48 if compressed else 96) * count)
        fn = self._lib.kzg_srs_read_compressed if compressed else self._lib.kzg_srs_read
        self._chk(fn(self._h, window, first, count, out))
        return out.raw

    # ------------------------------------------------------------------ hot path
    def commit(self, i: int, row_be32: bytes, evaluation_form: bool = True) -> bytes:
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_commit(self._h, i, row_be32, len(row_be32) // 32, int(evaluation_form), out))
        return out.raw

    def open(self, i: int, row_be32: bytes, alpha_be32: bytes, evaluation_form: bool = True) -> Tuple[bytes, bytes]:
        ev, pf = ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_open(self._h, i, row_be32, len(row_be32) // 32, int(evaluation_form), alpha_be32, ev, pf))
        return ev.raw, pf.raw

    def commit_open(self, i: int, row_be32: bytes, alpha_be32: bytes,
                    evaluation_form: bool = True) -> Tuple[bytes, bytes, bytes]:
        c, ev, pf = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_commit_open(self._h, i, row_be32, len(row_be32) // 32, int(evaluation_form),
                                            alpha_be32, c, ev, pf))
        return c.raw, ev.raw, pf.raw

    def commit_open_batch(self, i: int, rows_be32: Sequence[bytes], alpha_be32: bytes, gamma_be32: bytes,
                          evaluation_form: bool = True) -> Tuple[List[bytes], List[bytes], bytes]:
        """k rows of worker i opened at alpha with ONE proof for sum_j gamma^j f_j (kzg_commit_open_batch): returns
        ([C_j], [y_j], pi).  gamma must come from the verifier after the commitments are fixed (the library derives none)."""
        k = len(rows_be32)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"commit_open_batch: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        if len({len(r) for r in rows_be32}) != 1 or len(rows_be32[0]) % 32:
            raise KzgError(_native.KZG_E_ARG, "commit_open_batch: rows of unequal length")
        T = len(rows_be32[0]) // 32
        return self._commit_open_batch(i, k, b"".join(rows_be32), T, alpha_be32, gamma_be32, evaluation_form)

    def commit_open_batch_joined(self, i: int, rows_be32: bytes, k: int, alpha_be32: bytes, gamma_be32: bytes,
                                 evaluation_form: bool = True) -> Tuple[List[bytes], List[bytes], bytes]:
        """commit_open_batch on rows already in the C-ABI layout (k rows of T elements, row-major, one buffer): no join,
        which at 2^20 x 16 rows costs more host time than the GPU work it feeds."""
        if k <= 0 or k > _native.KZG_MAX_BATCH_OPEN or len(rows_be32) % (32 * k):
            raise KzgError(_native.KZG_E_ARG, f"commit_open_batch: {len(rows_be32)} bytes are not {k} equal rows")
        return self._commit_open_batch(i, k, rows_be32, len(rows_be32) // (32 * k), alpha_be32, gamma_be32, evaluation_form)

    def _commit_open_batch(self, i, k, rows, T, alpha_be32, gamma_be32, evaluation_form):
        if len(alpha_be32) != 32 or len(gamma_be32) != 32:   # the C side reads exactly 32 bytes of each
            raise KzgError(_native.KZG_E_ARG, "commit_open_batch: alpha / gamma must be 32 bytes")
        c, ev, pf = ctypes.create_string_buffer(48 * k), ctypes.create_string_buffer(32 * k), ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_commit_open_batch(self._h, i, k, rows, T, int(evaluation_form), alpha_be32, gamma_be32,
                                                  c, ev, pf))
        return ([c.raw[48 * j:48 * j + 48] for j in range(k)], [ev.raw[32 * j:32 * j + 32] for j in range(k)], pf.raw)

    def commit_open_multi(self, i: int, rows_be32: Sequence[bytes], points_be32: Sequence[bytes],
                          opened: Sequence[Sequence[int]], gammas_be32: Sequence[bytes], evaluation_form: bool = True
                          ) -> Tuple[List[bytes], List[List[bytes]], List[bytes]]:
        """k rows of worker i opened at m <= 4 points (kzg_commit_open_multi): opened[p] lists the rows opened at
        points_be32[p] (strictly increasing), gammas_be32[p] is that point's challenge.  Returns ([C_j], [[y_{j,p} for j in
        opened[p]] for p], [pi_p]).  The points and gammas must come from the verifier after the commitments are fixed."""
        k = len(rows_be32)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"commit_open_multi: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        if len({len(r) for r in rows_be32}) != 1 or len(rows_be32[0]) % 32:
            raise KzgError(_native.KZG_E_ARG, "commit_open_multi: rows of unequal length")
        T = len(rows_be32[0]) // 32
        return self._commit_open_multi(i, k, b"".join(rows_be32), T, points_be32, opened, gammas_be32, evaluation_form)

    def commit_open_multi_joined(self, i: int, rows_be32: bytes, k: int, points_be32: Sequence[bytes],
                                 opened: Sequence[Sequence[int]], gammas_be32: Sequence[bytes], evaluation_form: bool = True
                                 ) -> Tuple[List[bytes], List[List[bytes]], List[bytes]]:
        """commit_open_multi on rows already in the C-ABI layout (k rows of T elements, row-major, one buffer): no join."""
        if k <= 0 or k > _native.KZG_MAX_BATCH_OPEN or len(rows_be32) % (32 * k):
            raise KzgError(_native.KZG_E_ARG, f"commit_open_multi: {len(rows_be32)} bytes are not {k} equal rows")
        return self._commit_open_multi(i, k, rows_be32, len(rows_be32) // (32 * k), points_be32, opened, gammas_be32,
                                       evaluation_form)

    def _commit_open_multi(self, i, k, rows, T, points_be32, opened, gammas_be32, evaluation_form):
        masks, npairs = _native.open_masks(opened, k)
        m = len(opened)
        if len(points_be32) != m or len(gammas_be32) != m or any(len(x) != 32 for x in list(points_be32) + list(gammas_be32)):
            raise KzgError(_native.KZG_E_ARG, "commit_open_multi: one 32-byte point and gamma per opened list")
        c, ev, pf = (ctypes.create_string_buffer(48 * k), ctypes.create_string_buffer(32 * npairs),
                     ctypes.create_string_buffer(48 * m))
        self._chk(self._lib.kzg_commit_open_multi(self._h, i, k, rows, T, int(evaluation_form), m, b"".join(points_be32),
                                                  masks, b"".join(gammas_be32), c, ev, pf))
        evals, t = [], 0
        for rws in opened:
            evals.append([ev.raw[32 * (t + u):32 * (t + u) + 32] for u in range(len(rws))])
            t += len(rws)
        return [c.raw[48 * j:48 * j + 48] for j in range(k)], evals, [pf.raw[48 * p:48 * p + 48] for p in range(m)]

    # ---- committed row sets: commit rows once (kzg_rows_commit), open them later (kzg_rows_open), the shape of a
    # Fiat-Shamir prover that hashes its commitments before it draws the points and gammas
    def commit_rows(self, i: int, rows_be32: Sequence[bytes], evaluation_form: bool = True) -> "RowSet":
        """k <= 16 rows of worker i committed and kept on the device: a RowSet (handle, i, k, T, commitments), to be opened
        by open_rows any number of times and released with RowSet.release() (or as a context manager)."""
        k = len(rows_be32)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"commit_rows: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        if len({len(r) for r in rows_be32}) != 1 or len(rows_be32[0]) % 32:
            raise KzgError(_native.KZG_E_ARG, "commit_rows: rows of unequal length")
        T = len(rows_be32[0]) // 32
        return self._commit_rows(i, k, b"".join(rows_be32), T, evaluation_form)

    def _commit_rows(self, i, k, rows, T, evaluation_form):
        c, h = ctypes.create_string_buffer(48 * k), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit(self._h, i, k, rows, T, int(evaluation_form), c, ctypes.byref(h)))
        return RowSet(self, h.value, i, k, T, [c.raw[48 * j:48 * j + 48] for j in range(k)])

    # ---- typed columns in, cells of resident rows back out
    def commit_rows_typed(self, i: int, columns: Sequence[object], evaluation_form: bool = True,
                          T: Optional[int] = None) -> "RowSet":
        """commit_rows whose rows arrive as integer columns of their natural width (kzg_rows_commit_typed): each of the k <=
        16 columns is a buffer or a (buffer, fill_be32_or_None) pair -- see typed_column for the buffers taken; a bytes column
        holds 32-byte big-endian scalars, so one call can mix kinds.  T defaults to the longest column; a shorter column's
        cells [len, T) take its fill (None: 0).  A negative cell x of a signed column is r - |x|.  The set is the one
        commit_rows makes of the same values; only len * width bytes per column cross the host link."""
        what = "commit_rows_typed"
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        k = len(columns)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        cols = [typed_column(c, what) for c in columns]
        longest = max(n for _, n, _, _ in cols)
        if T is None:
            T = longest
        if isinstance(T, bool) or not isinstance(T, int) or T < 1:
            raise bad("T must be a positive integer (default: the longest column, which must not be empty)")
        if longest > T:
            raise bad(f"a column holds {longest} cells, more than T = {T}")
        arr, keep = (_native.Col * k)(), []
        for c, (kind, n, mv, fill) in enumerate(cols):
            if n == 0:
                ptr = None
            elif mv.readonly:   # ctypes takes no address of a read-only buffer: bytes that the view covers whole, else a copy
                whole = isinstance(mv.obj, bytes) and mv.nbytes == len(mv.obj)
                raw = mv.obj if whole else mv.tobytes()
                keep.append(raw)
                ptr = ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p)
            else:
                keep.append(mv)
                ptr = ctypes.c_void_p(ctypes.addressof(ctypes.c_char.from_buffer(mv)))
            arr[c].data, arr[c].count, arr[c].kind = ptr, n, kind
            arr[c].fill_be32 = None if fill is None else bytes(fill)
        c48, h = ctypes.create_string_buffer(48 * k), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_typed(self._h, i, k, arr, T, int(bool(evaluation_form)), c48, ctypes.byref(h)))
        del keep
        return RowSet(self, h.value, i, k, T, [c48.raw[48 * j:48 * j + 48] for j in range(k)])

    def read_rows(self, sets: Sequence[object], row: int, first: int, count: int, kind,
                  evaluation_form: bool = True) -> Tuple[bytes, int, Optional[int]]:
        """Cells [first, first + count) of row `row` of the concatenated sets (kzg_rows_read), as the values on the domain
        (evaluation_form, the default: what was uploaded or built) or the coefficients.  kind: a KZG_COL_* value or its name
        ("fr", "u8", "u16", "u32", "u64", "i32", "i64").  Returns (bytes, overflow, first_overflow): 32 big-endian bytes per cell
        for "fr", else native little-endian integers of the kind's width; a value >= r - 2^(w-1) reads as negative for the
        signed kinds; a cell that does not fit reads 0 and is counted in `overflow`, first_overflow being the smallest such row
        index (None: none).  The sets are unchanged."""
        what = "read_rows"
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        kind = _native.COL_DTYPES.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(kind, bool) or kind not in _native.COL_KINDS:
            raise bad(f"kind must be a KZG_COL_* value or one of {sorted(_native.COL_DTYPES)}")
        if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64 for v in (first, count)):
            raise bad("first and count must be integers in [0, 2^64)")
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"row must be an integer in [0, {_native.KZG_MAX_BATCH_OPEN})")
        n, hs = self._handle_array(sets, what)
        known = [self._set_len.get(int(getattr(x, "handle", x))) for x in sets]
        if all(v is not None for v in known) and first + count > min(v[1] for v in known):
            raise bad("first + count exceeds the row length")   # (before the output buffer is sized by a caller's count)
        width = _native.COL_KINDS[kind][0]
        if count > 1 << 32:   # (no row is that long: refused here, before a caller's count sizes the output buffer)
            raise bad("first + count exceeds the row length")
        try:
            out = ctypes.create_string_buffer(max(count * width, 1))
        except (MemoryError, OverflowError):
            raise bad(f"no room for {count} cells of {width} bytes: count exceeds any row this host can hold") from None
        ovf = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.kzg_rows_read(self._h, n, hs, row, first, count, kind, int(bool(evaluation_form)), out, ovf))
        return out.raw[:count * width], int(ovf[0]), None if int(ovf[1]) == _native.KZG_READ_NONE else int(ovf[1])

    def open_rows(self, sets: Sequence[object], points_be32: Sequence[bytes], opened: Sequence[Sequence[int]],
                  gammas_be32: Sequence[bytes]) -> Tuple[List[List[bytes]], List[bytes]]:
        """Opens committed sets (RowSet objects or bare handles) at m <= 4 points: their rows are numbered by
        concatenation in the order given, opened[p] lists point p's rows (as in commit_open_multi).  Returns
        ([[y_{j,p} for j in opened[p]] for p], [pi_p]), byte-identical to commit_open_multi on the concatenated rows."""
        handles = [int(getattr(x, "handle", x)) for x in sets]
        n = len(handles)
        if n == 0 or n > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"open_rows: {n} sets, expected 1 .. {_native.KZG_MAX_BATCH_OPEN}")
        hs = (ctypes.c_uint64 * n)(*handles)
        return self._open_rows_call(lambda *a: self._lib.kzg_rows_open(self._h, n, hs, *a), self._rows_of(sets),
                                    points_be32, opened, gammas_be32)

    def _rows_of(self, sets) -> int:
        """rows of the concatenation when every entry is a RowSet (a bare handle: checked by the library only)"""
        ks = [getattr(x, "k", None) for x in sets]
        return sum(ks) if all(k is not None for k in ks) else _native.KZG_MAX_BATCH_OPEN

    def _open_rows_call(self, call, k, points_be32, opened, gammas_be32):
        masks, npairs = _native.open_masks(opened, k)
        m = len(opened)
        if len(points_be32) != m or len(gammas_be32) != m or any(len(x) != 32 for x in list(points_be32) + list(gammas_be32)):
            raise KzgError(_native.KZG_E_ARG, "open_rows: one 32-byte point and gamma per opened list")
        ev, pf = ctypes.create_string_buffer(32 * npairs), ctypes.create_string_buffer(48 * m)
        self._chk(call(m, b"".join(points_be32), masks, b"".join(gammas_be32), ev, pf))
        evals, t = [], 0
        for rws in opened:
            evals.append([ev.raw[32 * (t + u):32 * (t + u) + 32] for u in range(len(rws))])
            t += len(rws)
        return evals, [pf.raw[48 * p:48 * p + 48] for p in range(m)]

    # ---- evaluate first, then open caller-weighted combinations: a Fiat-Shamir prover hashes the evaluations of eval_rows
    # before it derives the scalars it hands to open_rows_lincomb
    def eval_rows(self, sets: Sequence[object], points_be32: Sequence[bytes],
                  opened: Sequence[Sequence[int]]) -> List[List[bytes]]:
        """The evaluations of committed sets at m <= 4 points (kzg_rows_eval), no proof: rows numbered and `opened` as in
        open_rows.  Returns [[y_{j,p} for j in opened[p]] for p], byte-identical to open_rows' evaluations."""
        n, hs = self._handle_array(sets, "eval_rows")
        masks, npairs = _native.open_masks(opened, self._rows_of(sets))
        m = len(opened)
        if len(points_be32) != m or any(len(x) != 32 for x in points_be32):
            raise KzgError(_native.KZG_E_ARG, "eval_rows: one 32-byte point per opened list")
        ev = ctypes.create_string_buffer(32 * npairs)
        self._chk(self._lib.kzg_rows_eval(self._h, n, hs, m, b"".join(points_be32), masks, ev))
        evals, t = [], 0
        for rws in opened:
            evals.append([ev.raw[32 * (t + u):32 * (t + u) + 32] for u in range(len(rws))])
            t += len(rws)
        return evals

    def open_rows_lincomb(self, sets: Sequence[object], points_be32: Sequence[bytes],
                          coeffs: Sequence[Sequence[bytes]]) -> Tuple[List[bytes], List[bytes]]:
        """One proof per point for h_p = sum_j coeffs[p][j] f_j over the k concatenated rows of committed sets
        (kzg_rows_open_lincomb): coeffs[p] holds k 32-byte scalars (zero leaves a row out).  Returns ([v_p = h_p(alpha_p)],
        [pi_p]); verify_open_lincomb checks them against the sets' commitments."""
        n, hs = self._handle_array(sets, "open_rows_lincomb")
        m = len(points_be32)
        if m == 0 or m > _native.KZG_MAX_OPEN_POINTS or len(coeffs) != m:
            raise KzgError(_native.KZG_E_ARG, f"open_rows_lincomb: {m} points and {len(coeffs)} coefficient lists, "
                                              f"expected 1 .. {_native.KZG_MAX_OPEN_POINTS} of each")
        k = len(coeffs[0])
        if any(len(c) != k for c in coeffs) or any(len(x) != 32 for x in list(points_be32) + [c for cs in coeffs for c in cs]):
            raise KzgError(_native.KZG_E_ARG, "open_rows_lincomb: one 32-byte point and k 32-byte coefficients per point")
        vals, pf = ctypes.create_string_buffer(32 * m), ctypes.create_string_buffer(48 * m)
        self._chk(self._lib.kzg_rows_open_lincomb(self._h, n, hs, k, m, b"".join(points_be32),
                                                  b"".join(c for cs in coeffs for c in cs), vals, pf))
        return [vals.raw[32 * p:32 * p + 32] for p in range(m)], [pf.raw[48 * p:48 * p + 48] for p in range(m)]

    # ---- SHPLONK: one proof pair for any number of points.  Round A commits h on the device as a new one-row set; round B is
    # host arithmetic (shplonk_finish_coeffs) and open_rows_lincomb over the rows followed by h at the single point u
    def commit_shplonk(self, sets: Sequence[object], points_be32: Sequence[bytes], opened: Sequence[Sequence[int]],
                       coeffs_be32: Sequence[bytes]) -> Tuple[bytes, "RowSet"]:
        """Round A (kzg_rows_commit_shplonk): h = sum_j c_j (f_j - r_j) / Z_{S_j} over the k concatenated rows of committed
        sets, opened[p] the rows opened at point p (as in eval_rows; up to 8 distinct points), coeffs_be32 the k row scalars
        c_j (zero leaves a row out).  Returns (W = [h], a one-row RowSet holding h).  The c_j must be drawn after the
        commitments and the evaluations of eval_rows are fixed."""
        n, hs = self._handle_array(sets, "commit_shplonk")
        k, m = len(coeffs_be32), len(points_be32)
        if k == 0 or k > _native.KZG_MAX_SHPLONK_ROWS:
            raise KzgError(_native.KZG_E_ARG, f"commit_shplonk: k = {k} outside [1, {_native.KZG_MAX_SHPLONK_ROWS}]")
        masks, _ = _native.shplonk_masks(opened, k)
        if len(opened) != m or any(len(x) != 32 for x in list(points_be32) + list(coeffs_be32)):
            raise KzgError(_native.KZG_E_ARG, "commit_shplonk: one 32-byte point per opened list and k 32-byte coefficients")
        c, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_shplonk(self._h, n, hs, k, m, b"".join(points_be32), masks, b"".join(coeffs_be32),
                                                    c, ctypes.byref(h)))
        src = next((x for x in sets if hasattr(x, "T")), None)
        return c.raw, RowSet(self, h.value, getattr(src, "i", None), 1, getattr(src, "T", None), [c.raw])

    def open_shplonk_finish(self, sets: Sequence[object], h_set: object, points_be32: Sequence[bytes],
                            opened: Sequence[Sequence[int]], coeffs_be32: Sequence[bytes], u_be32: bytes) -> Tuple[bytes, bytes]:
        """Round B: (v, pi) of the opening of sum_j lambda_j f_j + lambda_k h at u, lambda from shplonk_finish_coeffs.  u must
        be drawn after W and must not be one of the points.  The proof is (W, pi)."""
        try:
            lam = shplonk_finish_coeffs(points_be32, opened, coeffs_be32, u_be32)
        except ValueError as e:
            raise KzgError(_native.KZG_E_ARG, f"open_shplonk_finish: {e}") from e
        vals, pfs = self.open_rows_lincomb(list(sets) + [h_set], [u_be32], [lam])
        return vals[0], pfs[0]

    def verify_open_shplonk(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                            opened: Sequence[Sequence[int]], coeffs32: Sequence[bytes], evals32: Sequence[Sequence[bytes]],
                            w48: bytes, u32: bytes, proof48: bytes) -> bool:
        """Pairing check of one SHPLONK opening (commit_shplonk + open_shplonk_finish) against resident slice i."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify_open_shplonk(i, commitments48, points32, opened, coeffs32, evals32, w48, u32, proof48)

    # ---- a set built from sets: the permutation grand product (PLONK round 2), computed and committed on the device
    def commit_grand_product(self, wire_sets: Sequence[object], sigma_sets: Sequence[object], shifts_be32: Sequence[bytes],
                             beta_be32: bytes, gamma_be32: bytes) -> Tuple["RowSet", bytes]:
        """z of kzg_rows_commit_grand_product over the k concatenated rows of wire_sets and of sigma_sets (RowSet objects or
        bare handles), one 32-byte shift per row.  Returns (a one-row RowSet holding z, the closing value as 32 bytes
        big-endian: 1 when the permutation holds).  beta and gamma must be drawn after the wire commitments are fixed."""
        return self._grand_product("commit_grand_product", wire_sets, sigma_sets, shifts_be32, beta_be32, gamma_be32)

    def _grand_product(self, what, wire_sets, sigma_sets, shifts_be32, beta_be32, gamma_be32, blind=None, start_be32=None):
        """The one body of commit_grand_product / _zk / _chain: `what` names the public method (and the native export
        kzg_rows_ + its suffix); blind = (usable, tail_be32) for the _zk and _chain forms, start_be32 for the _chain form."""
        nw, hw = self._handle_array(wire_sets, f"{what} (wires)")
        ns, hs = self._handle_array(sigma_sets, f"{what} (sigmas)")
        k, start = len(shifts_be32), [] if start_be32 is None else [start_be32]
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN or \
                any(len(x) != 32 for x in list(shifts_be32) + [beta_be32, gamma_be32] + start):
            raise KzgError(_native.KZG_E_ARG, f"{what}: 1 .. {_native.KZG_MAX_BATCH_OPEN} shifts, " +
                           ("beta, gamma and start" if start else "beta and gamma") + " of 32 bytes each")
        sets = list(wire_sets) + list(sigma_sets)
        extra, wi, T = self._layout_args(what, sets, blind)
        c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        self._chk(getattr(self._lib, "kzg_rows_" + what)(self._h, nw, hw, ns, hs, k, b"".join(shifts_be32), beta_be32, gamma_be32,
                                                         *extra, *start, c, cl, ctypes.byref(h)))
        return RowSet(self, h.value, wi, 1, T, [c.raw]), cl.raw

    # ---- a fourth set built from sets: the running sum of a logUp lookup argument, computed and committed on the device
    def commit_lookup_sum(self, input_sets: Sequence[object], table_sets: Sequence[object], mult_set: object, n_lookups: int,
                          width: int, theta_be32: bytes, beta_be32: bytes) -> Tuple["RowSet", bytes]:
        """S of kzg_rows_commit_lookup_sum: the n_lookups * width concatenated rows of input_sets (lookup-major) looked up in
        the width concatenated rows of table_sets with the multiplicities of the one-row mult_set (RowSet objects or bare
        handles).  Returns (a one-row RowSet holding S, the closing value as 32 bytes big-endian: 0 when the sum closes).
        theta and beta must be drawn after the commitments of the inputs, the table and the multiplicities are fixed."""
        return self._lookup_sum("commit_lookup_sum", input_sets, table_sets, mult_set, n_lookups, width, theta_be32, beta_be32)

    def _lookup_sum(self, what, input_sets, table_sets, mult_set, n_lookups, width, theta_be32, beta_be32, blind=None, sel=None):
        """The one body of commit_lookup_sum / _zk / _sel: blind = (usable, tail_be32) for the _zk and _sel forms, sel =
        (sel_sets, sel_index) for the _sel form."""
        ni, hi = self._handle_array(input_sets, f"{what} (inputs)")
        nt, ht = self._handle_array(table_sets, f"{what} (table)")
        _, hm = self._handle_array([mult_set], f"{what} (multiplicities)")
        if n_lookups < 1 or width < 1 or n_lookups * width > _native.KZG_MAX_BATCH_OPEN or len(theta_be32) != 32 \
                or len(beta_be32) != 32:
            raise KzgError(_native.KZG_E_ARG, f"{what}: n_lookups, width >= 1, n_lookups * width <= "
                                              f"{_native.KZG_MAX_BATCH_OPEN}, theta and beta of 32 bytes each")
        selargs = self._sel_args(what, *sel, n_lookups) if sel else ()
        extra, wi, T = self._layout_args(what, list(input_sets) + list(table_sets) + [mult_set], blind, sel_usable=bool(sel))
        c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        self._chk(getattr(self._lib, "kzg_rows_" + what)(self._h, ni, hi, nt, ht, hm[0], *selargs, n_lookups, width, theta_be32,
                                                         beta_be32, *extra, c, cl, ctypes.byref(h)))
        return RowSet(self, h.value, wi, 1, T, [c.raw]), cl.raw

    # ---- a fifth set built from sets: the multiplicity row of the lookup argument, joined and committed on the device
    def commit_multiplicities(self, input_sets: Sequence[object], table_sets: Sequence[object], n_lookups: int,
                              width: int) -> Tuple["RowSet", int]:
        """m of kzg_rows_commit_multiplicities: how many of the n_lookups * width concatenated rows' cells (input_sets,
        lookup-major) hit each row of the width concatenated rows of table_sets, every hit of a repeated table tuple counted
        on its first copy (RowSet objects or bare handles).  Returns (a one-row RowSet holding m, missing): missing is the
        number of cells whose tuple is no table row, 0 when every lookup is satisfied.  No challenge is involved: m is
        committed before theta and beta are drawn."""
        return self._multiplicities("commit_multiplicities", input_sets, table_sets, n_lookups, width)

    def _multiplicities(self, what, input_sets, table_sets, n_lookups, width, blind=None, sel=None):
        """The one body of commit_multiplicities / _zk / _sel: blind and sel as for _lookup_sum."""
        ni, hi = self._handle_array(input_sets, f"{what} (inputs)")
        nt, ht = self._handle_array(table_sets, f"{what} (table)")
        if n_lookups < 1 or width < 1 or n_lookups * width > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"{what}: n_lookups, width >= 1, n_lookups * width <= "
                                              f"{_native.KZG_MAX_BATCH_OPEN}")
        selargs = self._sel_args(what, *sel, n_lookups) if sel else ()
        extra, wi, T = self._layout_args(what, list(input_sets) + list(table_sets), blind, sel_usable=bool(sel))
        c, miss, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(getattr(self._lib, "kzg_rows_" + what)(self._h, ni, hi, nt, ht, *selargs, n_lookups, width, *extra, c,
                                                         ctypes.byref(miss), ctypes.byref(h)))
        return RowSet(self, h.value, wi, 1, T, [c.raw]), int(miss.value)

    # ---- the three builders above with blinding rows (kzg_rows_commit_*_zk): rows [0, usable) carry the circuit, row `usable`
    # closes the running value, the rows behind take the caller's random tail (T - usable - 1 scalars of 32 bytes)
    def _blind_args(self, what: str, sets, usable: int, tail_be32: Sequence[bytes]):
        """(usable, the tail's bytes or None, worker, T).  The native call reads T - usable - 1 scalars, so the tail's length
        is checked here against the row length, which a RowSet carries and the engine remembers for a bare handle."""
        src = next((x for x in sets if getattr(x, "T", None) is not None), None)
        i, T = (src.i, src.T) if src is not None else next(
            (self._set_len[int(x)] for x in sets if not hasattr(x, "handle") and int(x) in self._set_len), (None, None))
        tail = [bytes(x) for x in (tail_be32 or [])]
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        if T is None:
            raise bad("the row length of the sets is unknown to this engine (they were not committed through it)")
        if not isinstance(usable, int) or not 0 <= usable < 1 << 64 or any(len(x) != 32 for x in tail):
            raise bad("usable must be a non-negative integer and the tail scalars of 32 bytes each")
        if 1 <= usable < T and T - usable <= _native.KZG_MAX_BLIND_ROWS and len(tail) != T - usable - 1:
            raise bad(f"the tail must hold exactly T - usable - 1 = {T - usable - 1} scalars, not {len(tail)}")
        return usable, (b"".join(tail) if tail else None), i, T

    def _layout_args(self, what, sets, blind, sel_usable=False):
        """((usable, tail) for the native call, worker, T) of a builder over `sets`.  blind = None is the plain form: no extra
        argument, and bare handles whose row length the engine does not know are accepted (worker and T are None then)."""
        if blind is None:
            src = next((x for x in sets if hasattr(x, "T")), None)
            return (), getattr(src, "i", None), getattr(src, "T", None)
        usable, tail_be32 = blind
        usable, tail, wi, T = self._blind_args(what, sets, self._sel_usable(sets, usable) if sel_usable else usable, tail_be32)
        return (usable, tail), wi, T

    def commit_grand_product_zk(self, wire_sets: Sequence[object], sigma_sets: Sequence[object], shifts_be32: Sequence[bytes],
                                beta_be32: bytes, gamma_be32: bytes, usable: int,
                                tail_be32: Sequence[bytes] = ()) -> Tuple["RowSet", bytes]:
        """commit_grand_product over the first `usable` rows (kzg_rows_commit_grand_product_zk): z(w^usable) is the closing
        value (1 when the permutation holds on the usable rows), rows usable + 1 .. T - 1 of z are tail_be32.  """
        return self._grand_product("commit_grand_product_zk", wire_sets, sigma_sets, shifts_be32, beta_be32, gamma_be32,
                                   (usable, tail_be32))

    def commit_lookup_sum_zk(self, input_sets: Sequence[object], table_sets: Sequence[object], mult_set: object, n_lookups: int,
                             width: int, theta_be32: bytes, beta_be32: bytes, usable: int,
                             tail_be32: Sequence[bytes] = ()) -> Tuple["RowSet", bytes]:
        """commit_lookup_sum over the first `usable` rows (kzg_rows_commit_lookup_sum_zk): S(w^usable) is the closing value
        (0 when the sum closes on the usable rows), rows usable + 1 .. T - 1 of S are tail_be32."""
        return self._lookup_sum("commit_lookup_sum_zk", input_sets, table_sets, mult_set, n_lookups, width, theta_be32, beta_be32,
                                (usable, tail_be32))

    def commit_multiplicities_zk(self, input_sets: Sequence[object], table_sets: Sequence[object], n_lookups: int, width: int,
                                 usable: int, tail_be32: Sequence[bytes] = ()) -> Tuple["RowSet", int]:
        """commit_multiplicities over the first `usable` table rows and input cells (kzg_rows_commit_multiplicities_zk):
        m(w^usable) = 0, rows usable + 1 .. T - 1 of m are tail_be32; missing counts usable cells only."""
        return self._multiplicities("commit_multiplicities_zk", input_sets, table_sets, n_lookups, width, (usable, tail_be32))

    # ---- the two lookup builders with per-row selectors (kzg_rows_commit_*_sel): sel_index[l] is None (no selector) or the
    # index of lookup l's selector row in the concatenated rows of sel_sets; usable = None is the plain layout (no closing row),
    # anything else the _zk one
    def _sel_args(self, what: str, sel_sets, sel_index, n_lookups: int):
        """(n_sel_handles, the handle array or None, the index array)."""
        sel_sets = list(sel_sets or [])
        idx = [_native.KZG_NO_SELECTOR if j is None else j for j in sel_index]
        if len(idx) != n_lookups or any(not isinstance(j, int) or not 0 <= j <= _native.KZG_NO_SELECTOR for j in idx):
            raise KzgError(_native.KZG_E_ARG, f"{what}: sel_index must hold n_lookups entries, each None or a row index")
        ns, hs = self._handle_array(sel_sets, f"{what} (selectors)") if sel_sets else (0, None)
        return ns, hs, (ctypes.c_uint32 * n_lookups)(*idx)

    def commit_lookup_sum_sel(self, input_sets: Sequence[object], table_sets: Sequence[object], mult_set: object,
                              sel_sets: Sequence[object], sel_index: Sequence[Optional[int]], n_lookups: int, width: int,
                              theta_be32: bytes, beta_be32: bytes, usable: Optional[int] = None,
                              tail_be32: Sequence[bytes] = ()) -> Tuple["RowSet", bytes]:
        """commit_lookup_sum / _zk with the numerator q_l of lookup l read from row sel_index[l] of the concatenated rows of
        sel_sets (kzg_rows_commit_lookup_sum_sel); None there is the constant 1.  The library does not judge q.  usable =
        None (the plain layout) needs the row length, which RowSet objects carry and the engine remembers for the handles of
        sets committed through it: with bare handles of other origin pass usable = T yourself."""
        return self._lookup_sum("commit_lookup_sum_sel", input_sets, table_sets, mult_set, n_lookups, width, theta_be32, beta_be32,
                                (usable, tail_be32), (sel_sets, sel_index))

    def commit_multiplicities_sel(self, input_sets: Sequence[object], table_sets: Sequence[object], sel_sets: Sequence[object],
                                  sel_index: Sequence[Optional[int]], n_lookups: int, width: int, usable: Optional[int] = None,
                                  tail_be32: Sequence[bytes] = ()) -> Tuple["RowSet", int]:
        """commit_multiplicities / _zk over the cells whose selector is not zero (kzg_rows_commit_multiplicities_sel):
        sel_index[l] names lookup l's selector row in the concatenated rows of sel_sets, None probes every cell.  usable =
        None: as for commit_lookup_sum_sel."""
        return self._multiplicities("commit_multiplicities_sel", input_sets, table_sets, n_lookups, width, (usable, tail_be32),
                                    (sel_sets, sel_index))

    def _sel_usable(self, sets, usable):
        """usable = None (the plain layout) is the row length, which the native call expects in its place."""
        if usable is not None:
            return usable
        src = next((x for x in sets if getattr(x, "T", None) is not None), None)
        T = src.T if src is not None else next(
            (self._set_len[int(x)][1] for x in sets if not hasattr(x, "handle") and int(x) in self._set_len), None)
        if T is None:
            raise KzgError(_native.KZG_E_ARG, "commit_*_sel: the row length of the sets is unknown to this engine (they were "
                                              "not committed through it)")
        return T

    # ---- a set built from sets: the running product of a shuffle argument.  ONE call for every form: selectors and blinding
    # rows are optional arguments (kzg_shuffle_opts)
    def commit_shuffle(self, input_sets: Sequence[object], shuffle_sets: Sequence[object], n_groups: int, width: int,
                       theta_be32: bytes, gamma_be32: bytes, sel_sets: Optional[Sequence[object]] = None,
                       input_sel: Optional[Sequence[Optional[int]]] = None,
                       shuffle_sel: Optional[Sequence[Optional[int]]] = None, usable: Optional[int] = None,
                       tail: Sequence[bytes] = ()) -> Tuple["RowSet", bytes]:
        """z of kzg_rows_commit_shuffle: the n_groups * width concatenated rows of input_sets (group-major) against as many of
        shuffle_sets (RowSet objects or bare handles).  input_sel / shuffle_sel: None, or one entry per group, None or the
        index of that side's selector row in the concatenated rows of sel_sets.  usable = None is the plain layout, anything
        else that of commit_grand_product_zk with its tail.  Returns (a one-row RowSet holding z, the closing value as 32
        bytes big-endian: 1 when the product closes).  theta and gamma must be drawn after the commitments of all input and
        shuffle rows are fixed; the argument is the relation shuffle_quotient_terms writes, not the closing value."""
        what = "commit_shuffle"
        ni, hi = self._handle_array(input_sets, f"{what} (inputs)")
        ns, hs = self._handle_array(shuffle_sets, f"{what} (shuffles)")
        if n_groups < 1 or width < 1 or n_groups * width > _native.KZG_MAX_BATCH_OPEN or len(theta_be32) != 32 \
                or len(gamma_be32) != 32:
            raise KzgError(_native.KZG_E_ARG, f"{what}: n_groups, width >= 1, n_groups * width <= "
                                              f"{_native.KZG_MAX_BATCH_OPEN}, theta and gamma of 32 bytes each")
        if usable == 0:   # (the C call reads 0 as "plain layout"; here that is None, and 0 is the _zk calls' range error)
            raise KzgError(_native.KZG_E_ARG, f"{what}: usable must be in [1, T - 1] (None: the plain layout)")
        opts = None
        if sel_sets or input_sel is not None or shuffle_sel is not None or usable is not None:
            opts = _native.ShuffleOpts()
            # (keep: the arrays must outlive the call)
            keep = [self._sel_args(what, sel_sets, [None] * n_groups if idx is None else idx, n_groups)
                    for idx in (input_sel, shuffle_sel)]
            opts.n_sel_handles, opts.sel_handles = keep[0][0], keep[0][1]
            if input_sel is not None:
                opts.input_sel = keep[0][2]
            if shuffle_sel is not None:
                opts.shuffle_sel = keep[1][2]
        blind = None if usable is None else (usable, tail)
        extra, wi, T = self._layout_args(what, list(input_sets) + list(shuffle_sets), blind)
        if extra:
            opts.usable, opts.tail_be32 = extra
        c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_shuffle(self._h, ni, hi, ns, hs, n_groups, width, theta_be32, gamma_be32,
                                                    ctypes.byref(opts) if opts is not None else None, c, cl, ctypes.byref(h)))
        return RowSet(self, h.value, wi, 1, T, [c.raw]), cl.raw

    # ---- a set built from sets: the columns of committed sets, stably sorted as tuples on the device (the second side of a
    # shuffle whose first side is those columns)
    def commit_sorted(self, input_sets: Sequence[object], width: int, n_keys: Optional[int] = None, usable: Optional[int] = None,
                      tail: Sequence[bytes] = ()) -> "RowSet":
        """kzg_rows_commit_sorted: the `width` concatenated rows of input_sets (RowSet objects or bare handles) are the columns
        of one tuple per row; the new RowSet of `width` rows holds the tuples sorted ascending by the canonical integers of the
        first n_keys columns (None: all of them), column 0 most significant, ties by source row.  usable = None sorts all T
        rows; otherwise only rows [0, usable) are sorted and row usable + s of column c takes tail[c * (T - usable) + s] (32
        bytes each, column-major; there is no closing row)."""
        what = "commit_sorted"
        ni, hi = self._handle_array(input_sets, what)
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        if n_keys is None:
            n_keys = width
        if not isinstance(width, int) or not 1 <= width <= _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"width must be in [1, {_native.KZG_MAX_BATCH_OPEN}]")
        if not isinstance(n_keys, int) or not 1 <= n_keys <= width:
            raise bad("n_keys must be in [1, width]")
        wi, T, lay = self._column_layout(what, input_sets, width, "width", "sorted", usable, tail)
        opts = _native.SortedOpts(*lay) if lay else None
        c, h = ctypes.create_string_buffer(48 * width), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_sorted(self._h, ni, hi, width, n_keys, ctypes.byref(opts) if opts is not None else None,
                                                   c, ctypes.byref(h)))
        return RowSet(self, h.value, wi, width, T, [c.raw[48 * p:48 * p + 48] for p in range(width)])

    # ---- a set built from sets: the permutation's sigma columns from variable labels, and the copy check over the same labels
    def _sigma_opts(self, what: str, usable, free_label):
        """kzg_sigma_opts (None for the plain layout without a free label) and the object that keeps its bytes alive"""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        if usable is not None and (isinstance(usable, bool) or not isinstance(usable, int) or not 1 <= usable < 1 << 64):
            raise bad("usable must be in [1, T - 1] (None: all T rows take part)")   # (the C call reads 0 as "plain layout")
        if free_label is not None:
            free_label = bytes(free_label)
            if len(free_label) != 32:
                raise bad("the free label must be of 32 bytes")
        if usable is None and free_label is None:
            return None
        return _native.SigmaOpts(usable or 0, free_label)

    def commit_sigma(self, label_sets: Sequence[object], shifts_be32: Sequence[bytes], usable: Optional[int] = None,
                     free_label: Optional[bytes] = None) -> Tuple[List[bytes], "RowSet", Dict[str, int]]:
        """kzg_rows_commit_sigma.  The concatenated rows of label_sets (RowSet objects or bare handles) are k = len(shifts_be32)
        label columns; cells with equal labels (as canonical integers) are one copy class.  The new RowSet of k rows holds the
        permutation in which every class is one cycle in ascending flat index c * T + t: sigma_c(w^t) = shifts[c'] * w^t' for
        the image (c', t').  usable = None: all T rows take part; otherwise rows [0, usable) do and the rows behind map to
        themselves, their labels unread.  A cell whose label is free_label (32 bytes; None: no such label) maps to itself.
        Returns (the k commitments, the RowSet -- the handle of the new set --, {"classes": distinct non-free labels among the
        participating cells, "fixed": participating cells that map to themselves})."""
        what = "commit_sigma"
        nl, hl = self._handle_array(label_sets, what)
        shifts = [bytes(x) for x in shifts_be32]
        k = len(shifts)
        if not 1 <= k <= _native.KZG_MAX_BATCH_OPEN or any(len(x) != 32 for x in shifts):
            raise KzgError(_native.KZG_E_ARG, f"{what}: 1 .. {_native.KZG_MAX_BATCH_OPEN} shifts of 32 bytes each")
        opts = self._sigma_opts(what, usable, free_label)
        wi, T, _ = self._column_layout(what, label_sets, k, "k", "linked", None, ())
        c, h, st = ctypes.create_string_buffer(48 * k), ctypes.c_uint64(0), (ctypes.c_uint64 * 2)()
        self._chk(self._lib.kzg_rows_commit_sigma(self._h, nl, hl, k, b"".join(shifts), ctypes.byref(opts) if opts is not None else None,
                                                  c, st, ctypes.byref(h)))
        rs = RowSet(self, h.value, wi, k, T, [c.raw[48 * p:48 * p + 48] for p in range(k)])
        return list(rs.commitments), rs, {"classes": int(st[0]), "fixed": int(st[1])}

    def check_copies(self, wire_sets: Sequence[object], label_sets: Sequence[object], usable: Optional[int] = None,
                     free_label: Optional[bytes] = None) -> Dict[str, object]:
        """kzg_rows_check_copies: the wire columns (the concatenated rows of wire_sets) against the copy classes of the label
        columns of commit_sigma, cell by cell on the device; both concatenations hold the same k rows, which must be known to
        this engine (sets committed through it).  A participating, non-free cell is a violation when its value differs from
        that of its class's smallest cell.  Returns {"violations": their number, "first": the (column, row) of the smallest
        violating flat index or None}.  Creates no set and runs no MSM; a count convinces no verifier."""
        what = "check_copies"
        nw, hw = self._handle_array(wire_sets, f"{what} (wires)")
        nl, hl = self._handle_array(label_sets, f"{what} (labels)")
        widths = [x.k if hasattr(x, "handle") else self._set_rows.get(int(x)) for x in label_sets]
        wi, T, _ = self._column_layout(what, list(label_sets) + list(wire_sets), 0, "k", "checked", None, ())
        if any(w is None for w in widths) or T is None:   # (k is an argument of the C call; T splits the flat index)
            raise KzgError(_native.KZG_E_ARG, f"{what}: the row count or length of the label sets is unknown to this engine "
                                              "(they were not committed through it)")
        k = sum(widths)
        if not 1 <= k <= _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"{what}: the label sets hold {k} rows, expected 1 .. {_native.KZG_MAX_BATCH_OPEN}")
        opts = self._sigma_opts(what, usable, free_label)
        out = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.kzg_rows_check_copies(self._h, nw, hw, nl, hl, k, ctypes.byref(opts) if opts is not None else None, out))
        first = None if int(out[1]) == 0xffffffffffffffff else (int(out[1]) // T, int(out[1]) % T)
        return {"violations": int(out[0]), "first": first}

    def _column_layout(self, what: str, input_sets, n_cols: int, cols_name: str, verb: str, usable, tail):
        """The usable layout WITHOUT a closing row (kzg_sorted_opts, kzg_derive_opts) of a builder with n_cols output columns:
        (worker, T, None for the plain layout or (usable, the column-major tail's bytes or None)); worker and T are None for
        bare handles of sets this engine did not commit, which only the plain layout accepts."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        tail = [bytes(x) for x in (tail or [])]
        src = next((x for x in input_sets if getattr(x, "T", None) is not None), None)
        wi, T = (src.i, src.T) if src is not None else next(
            (self._set_len[int(x)] for x in input_sets if not hasattr(x, "handle") and int(x) in self._set_len), (None, None))
        if usable is None:
            if tail:
                raise bad(f"a tail needs usable (None: all T rows are {verb})")
            return wi, T, None
        if not isinstance(usable, int) or not 1 <= usable < 1 << 64:   # (the C call reads 0 as "plain layout": here None)
            raise bad(f"usable must be in [1, T - 1] (None: all T rows are {verb})")
        if any(len(x) != 32 for x in tail):
            raise bad("the tail scalars must be of 32 bytes each")
        if T is None:
            raise bad("the row length of the sets is unknown to this engine (they were not committed through it)")
        if usable < T and T - usable <= _native.KZG_MAX_BLIND_ROWS and len(tail) != n_cols * (T - usable):
            raise bad(f"the tail must hold exactly {cols_name} * (T - usable) = {n_cols * (T - usable)} scalars, not {len(tail)}")
        return wi, T, (usable, b"".join(tail) if tail else None)

    # ---- a set built from sets: the helper columns of zero tests and range checks, each a function of one resident column
    def commit_derived(self, input_sets: Sequence[object], ops: Sequence[tuple], usable: Optional[int] = None,
                       tail: Sequence[bytes] = ()) -> Tuple["RowSet", List[int]]:
        """kzg_rows_commit_derived over the concatenated rows of input_sets (RowSet objects or bare handles).  ops: ("inv0", row)
        gives the row 1 / x, 0 where x = 0; ("inv0", row, True) also the bit row behind it (1 where x = 0); ("limbs", row, bits,
        count) the `count` limbs of `bits` bits of x's canonical integer, least significant first.  Returns (the new RowSet of
        all output rows in the order of ops, one count per op: the zero cells of an inv0 op, the cells at or above 2^(bits *
        count) of a limbs op).  usable = None reads all T rows; otherwise only rows [0, usable) are read and row usable + s of
        output column c takes tail[c * (T - usable) + s] (32 bytes each, column-major; there is no closing row)."""
        what = "commit_derived"
        ni, hi = self._handle_array(input_sets, what)
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        ops = list(ops) if isinstance(ops, (list, tuple)) else None
        if not ops:
            raise bad("ops must be a non-empty list")
        recs = []
        for op in ops:
            if not isinstance(op, (list, tuple)) or not op or op[0] not in ("inv0", "limbs"):
                raise bad('an op is ("inv0", row), ("inv0", row, True) or ("limbs", row, bits, count)')
            if op[0] == "inv0":
                if len(op) not in (2, 3) or (len(op) == 3 and not isinstance(op[2], bool)):
                    raise bad('an inv0 op is ("inv0", row) or ("inv0", row, with_bit)')
                kind, nums, count = _native.KZG_DERIVE_INV0, [op[1], 0], 2 if len(op) == 3 and op[2] else 1
            else:
                if len(op) != 4:
                    raise bad('a limbs op is ("limbs", row, bits, count)')
                kind, nums, count = _native.KZG_DERIVE_LIMBS, [op[1], op[2]], op[3]
            if any(not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 32 for v in nums + [count]):
                raise bad("row, bits and count must be integers in [0, 2^32)")
            if kind == _native.KZG_DERIVE_LIMBS and (not 1 <= nums[1] <= 32 or not 1 <= count <= _native.KZG_MAX_BATCH_OPEN
                                                     or nums[1] * count > 256):
                raise bad(f"bits must be in [1, 32], count in [1, {_native.KZG_MAX_BATCH_OPEN}] and bits * count at most 256")
            recs.append((kind, nums[0], nums[1], count))
        n_out = sum(r[3] for r in recs)
        if n_out > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"the ops give {n_out} output rows, at most {_native.KZG_MAX_BATCH_OPEN} fit one call")
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        arr =(_native.DeriveOp * len(recs))(*[_native.DeriveOp(*r) for r in recs])
        c, h, cnt = ctypes.create_string_buffer(48 * n_out), ctypes.c_uint64(0), (ctypes.c_uint64 * len(recs))()
        self._chk(self._lib.kzg_rows_commit_derived(self._h, ni, hi, len(recs), arr, ctypes.byref(opts) if opts is not None else None,
                                                    c, cnt, ctypes.byref(h)))
        return RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]), [int(v) for v in cnt]

    # ---- a set built from sets: machine-word arithmetic on the canonical integers of one or two resident columns
    _INT_KINDS = {"and": _native.KZG_INT_AND, "or": _native.KZG_INT_OR, "xor": _native.KZG_INT_XOR, "add": _native.KZG_INT_ADD,
                  "sub": _native.KZG_INT_SUB, "mul": _native.KZG_INT_MUL, "divmod": _native.KZG_INT_DIVMOD,
                  "split": _native.KZG_INT_SPLIT}

    @classmethod
    def int_ops(cls, ops, what: str = "commit_int") -> List[tuple]:
        """The kzg_int_op fields (kind, width, a, b, imm, flags, count) of a list of ops (kind, w, a, b) or (kind, w, a, b,
        count): kind one of "and" "or" "xor" "add" "sub" "mul" "divmod" "split", w in [1, 64], a a row index, b a row index or
        ("imm", value), count 1 or, except on the bitwise kinds, 2 (default 1).  Raises KzgError(KZG_E_ARG) with the cause."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: int: {why}")   # noqa: E731
        ops = list(ops) if isinstance(ops, (list, tuple)) else None
        if not ops or len(ops) > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"ops must be a list of 1 .. {_native.KZG_MAX_BATCH_OPEN} entries (n_ops)")
        is_u = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < top   # noqa: E731
        recs = []
        for op in ops:
            if not isinstance(op, (list, tuple)) or len(op) not in (4, 5):
                raise bad("an op is (kind, w, a, b) or (kind, w, a, b, count)")
            name, w, a, b = op[:4]
            count = op[4] if len(op) == 5 else 1
            if not isinstance(name, str) or name not in cls._INT_KINDS:
                raise bad(f"unknown kind {name!r} (one of {', '.join(cls._INT_KINDS)})")
            kind = cls._INT_KINDS[name]
            if not is_u(w, 65) or w == 0:
                raise bad("the width must be an integer in [1, 64]")
            if not is_u(count, 3) or count == 0 or (count == 2 and kind < _native.KZG_INT_ADD):
                raise bad("count must be 1 on and, or and xor, and 1 or 2 on the other kinds")
            if not is_u(a, 1 << 32):
                raise bad("a row must be an integer in [0, 2^32)")
            if isinstance(b, (list, tuple)):
                if len(b) != 2 or b[0] != "imm" or not is_u(b[1], 1 << 64):
                    raise bad('an immediate is ("imm", value) with value an integer in [0, 2^64)')
                if b[1] > w if kind == _native.KZG_INT_SPLIT else b[1] >> w:
                    raise bad("an immediate must be below 2^width (split: a shift of at most width)")
                recs.append((kind, w, a, 0, b[1], _native.KZG_INT_IMM, count))
            elif is_u(b, 1 << 32):
                recs.append((kind, w, a, b, 0, 0, count))
            else:
                raise bad('the second operand is a row, an integer in [0, 2^32), or ("imm", value)')
        if sum(r[6] for r in recs) > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"n_out: the ops give {sum(r[6] for r in recs)} output rows, at most {_native.KZG_MAX_BATCH_OPEN} fit one call")
        return recs

    def commit_int(self, input_sets: Sequence[object], ops: Sequence[tuple], usable: Optional[int] = None,
                   tail: Sequence[bytes] = ()) -> Tuple["RowSet", List[int], List[Optional[int]]]:
        """kzg_rows_commit_int over the concatenated rows of input_sets (RowSet objects or bare handles).  ops: see int_ops; the
        operands are the cells' canonical integers reduced to their low w bits, the output rows of an op in this order: and /
        or / xor: a op b; add: the sum mod 2^w, the carry; sub: the difference mod 2^w, the borrow (1 where a < b); mul: the low
        word, the high word; divmod: the quotient (2^w - 1 where b = 0), the remainder (a where b = 0); split: a >> s, a mod 2^s
        with s the second operand, at most w.  Returns (the new RowSet of all output rows in the order of ops; per op the number
        of cells read with an operand at or above 2^w (a split's shift cell: above w); per op the smallest such row, or None).
        usable = None reads all T rows; otherwise only rows [0, usable) are read and row usable + s of output column c takes
        tail[c * (T - usable) + s] (32 bytes each, column-major; there is no closing row)."""
        what = "commit_int"
        ni, hi = self._handle_array(input_sets, what)
        recs = self.int_ops(ops, what)
        n_out = sum(r[6] for r in recs)
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        arr = (_native.IntOp * len(recs))(*[_native.IntOp(*r) for r in recs])
        c, h = ctypes.create_string_buffer(48 * n_out), ctypes.c_uint64(0)
        cnt, first = (ctypes.c_uint64 * len(recs))(), (ctypes.c_uint64 * len(recs))()
        self._chk(self._lib.kzg_rows_commit_int(self._h, ni, hi, len(recs), arr, ctypes.byref(opts) if opts is not None else None,
                                                c, cnt, first, ctypes.byref(h)))
        return (RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]), [int(v) for v in cnt],
                [None if int(v) == _native.KZG_INT_NONE else int(v) for v in first])

    # ---- a set built from sets: the same arithmetic and its signed kinds, the kind chosen per row by an op-code column
    _ALU_KINDS = {name: num for num, name in enumerate(
        ("and", "or", "xor", "add", "sub", "mul", "divmod", "split", "ltu", "lt", "eq", "sll", "srl", "sra", "rotl", "rotr",
         "mulhu", "mulh", "mulhsu", "div", "rem", "remu", "sext"), 1)}

    @classmethod
    def alu_program(cls, program, what: str = "commit_alu") -> List[tuple]:
        """The kzg_alu_entry fields (kind, width, imm, flags, pad) of a program: a list of 1 .. 64 entries, the index the
        op-code, each None (idle), (kind, w) or (kind, w, ("imm", value)) with kind one of "and" "or" "xor" "add" "sub" "mul"
        "divmod" "split" "ltu" "lt" "eq" "sll" "srl" "sra" "rotl" "rotr" "mulhu" "mulh" "mulhsu" "div" "rem" "remu" "sext" and w
        in [1, 64].  An immediate is below 2^w; split's and sext's at most w, sext's not 0.  Raises KzgError(KZG_E_ARG)."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: alu: {why}")   # noqa: E731
        program = list(program) if isinstance(program, (list, tuple)) else None
        if not program or len(program) > _native.KZG_ALU_MAX_PROGRAM:
            raise bad(f"the program must be a list of 1 .. {_native.KZG_ALU_MAX_PROGRAM} entries (n_entries)")
        is_u = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < top   # noqa: E731
        recs = []
        for en in program:
            if en is None:
                recs.append((_native.KZG_ALU_IDLE, 0, 0, 0, 0))
                continue
            if not isinstance(en, (list, tuple)) or len(en) not in (2, 3):
                raise bad('an entry is None, (kind, w) or (kind, w, ("imm", value))')
            name, w = en[:2]
            if not isinstance(name, str) or name not in cls._ALU_KINDS:
                raise bad(f"unknown kind {name!r} (one of {', '.join(cls._ALU_KINDS)})")
            kind = cls._ALU_KINDS[name]
            if not is_u(w, 65) or w == 0:
                raise bad("the width must be an integer in [1, 64]")
            if len(en) == 2:
                recs.append((kind, w, 0, 0, 0))
                continue
            imm = en[2]
            if not isinstance(imm, (list, tuple)) or len(imm) != 2 or imm[0] != "imm" or not is_u(imm[1], 1 << 64):
                raise bad('an immediate is ("imm", value) with value an integer in [0, 2^64)')
            v = imm[1]
            if (v > w or (name == "sext" and v == 0)) if name in ("split", "sext") else v >> w:
                raise bad("an immediate must be below 2^width (split, sext: at most width; sext: at least 1)")
            recs.append((kind, w, v, _native.KZG_ALU_IMM, 0))
        return recs

    @classmethod
    def alu_units(cls, units, recs, what: str = "commit_alu") -> List[tuple]:
        """The kzg_alu_unit fields (op_row, a, b, count) of 1 .. 8 units (op_row, a, b) or (op_row, a, b, count), rows of the
        concatenated input sets, count 1 or 2 (default 1); recs: the program's fields from alu_program -- count 2 needs an entry
        whose kind has a second row.  Raises KzgError(KZG_E_ARG) with the cause."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: alu: {why}")   # noqa: E731
        units = list(units) if isinstance(units, (list, tuple)) else None
        if not units or len(units) > _native.KZG_ALU_MAX_UNITS:
            raise bad(f"units must be a list of 1 .. {_native.KZG_ALU_MAX_UNITS} entries (n_units)")
        is_u = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < top   # noqa: E731
        two_rows = any(r[0] > _native.KZG_ALU_XOR for r in recs)
        out = []
        for un in units:
            if not isinstance(un, (list, tuple)) or len(un) not in (3, 4):
                raise bad("a unit is (op_row, a, b) or (op_row, a, b, count)")
            count = un[3] if len(un) == 4 else 1
            if not all(is_u(v, 1 << 32) for v in un[:3]):
                raise bad("a row must be an integer in [0, 2^32)")
            if not is_u(count, 3) or count == 0 or (count == 2 and not two_rows):
                raise bad("count must be 1 or 2, and 1 where no entry's kind has a second row (and, or, xor)")
            out.append((un[0], un[1], un[2], count))
        if sum(u[3] for u in out) > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"n_out: the units give {sum(u[3] for u in out)} output rows, at most {_native.KZG_MAX_BATCH_OPEN} fit one call")
        return out

    def commit_alu(self, input_sets: Sequence[object], program: Sequence, units: Sequence[tuple], usable: Optional[int] = None,
                   tail: Sequence[bytes] = ()) -> Tuple["RowSet", dict]:
        """kzg_rows_commit_alu over the concatenated rows of input_sets (RowSet objects or bare handles): the machine-word
        arithmetic of commit_int with the kind chosen PER ROW.  program: see alu_program; units: see alu_units.  Cell t of a unit
        takes c, the canonical integer of op_row[t]: c beyond the program is unknown (outputs 0, counted), program[c] None is idle
        (outputs 0, nothing read or counted), otherwise the entry's kind acts on a[t] and b[t] (or the entry's immediate) reduced
        to their low w bits.  The rows of the kinds commit_int lacks, row 0 then row 1, with s = b mod w: ltu / lt / eq: the bit,
        (a - b) mod 2^w; sll: the low word, the bits shifted out; srl / sra: the shifted word, a mod 2^s; rotl / rotr: the
        rotated word, the wrapped bits; mulhu / mulh / mulhsu: the high word, the low word; div: quotient, remainder (RISC-V);
        rem: remainder, quotient; remu: remainder, quotient; sext: the low f bits sign-extended, bit f - 1.  Returns (the new
        RowSet of all output rows, unit by unit; {"counts", "first", "unknown", "first_unknown"}, per unit the cells read with an
        operand out of range and the cells with an unknown op-code, and the smallest such rows or None).  usable and tail: as
        for commit_int."""
        what = "commit_alu"
        ni, hi = self._handle_array(input_sets, what)
        recs = self.alu_program(program, what)
        urecs = self.alu_units(units, recs, what)
        n_out = sum(u[3] for u in urecs)
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        prog = (_native.AluEntry * len(recs))(*[_native.AluEntry(*r) for r in recs])
        arr = (_native.AluUnit * len(urecs))(*[_native.AluUnit(*u) for u in urecs])
        c, h = ctypes.create_string_buffer(48 * n_out), ctypes.c_uint64(0)
        nu = len(urecs)
        cnt, first, unk, funk = [(ctypes.c_uint64 * nu)() for _ in range(4)]
        self._chk(self._lib.kzg_rows_commit_alu(self._h, ni, hi, len(recs), prog, nu, arr,
                                                ctypes.byref(opts) if opts is not None else None, c, cnt, first, unk, funk,
                                                ctypes.byref(h)))
        none = lambda vs: [None if int(v) == _native.KZG_ALU_NONE else int(v) for v in vs]   # noqa: E731
        return (RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]),
                {"counts": [int(v) for v in cnt], "first": none(first), "unknown": [int(v) for v in unk],
                 "first_unknown": none(funk)})

    # ---- a set built from sets: multi-limb integers (256, 384, 512 bits) and a b + c mod m over runs of limb rows
    _WIDE_KINDS = {"add": _native.KZG_WIDE_ADD, "sub": _native.KZG_WIDE_SUB, "mul": _native.KZG_WIDE_MUL,
                   "divmod": _native.KZG_WIDE_DIVMOD, "mulmod": _native.KZG_WIDE_MULMOD, "carry": _native.KZG_WIDE_CARRY}
    _WIDE_KEYS = ("kind", "bits", "limbs", "a", "b", "c", "q", "r", "m", "neg_c", "count")

    @classmethod
    def wide_ops(cls, ops, what: str = "commit_wide") -> List[tuple]:
        """The kzg_wide_op fields (kind, bits, limbs, count, flags, a, b, c, q, r, imm_be64, m_be64) of a list of ops.  An op is
        a mapping: kind ("add" "sub" "mul" "divmod" "mulmod" "carry"), bits (b in [1, 64]; carry: 56), limbs (L in [1, 8], b L
        <= 512), a (the first row of operand a), b (a first row, ("imm", value) or None), and where the kind takes them c, q, r
        (first rows or None), m (the modulus), neg_c (bool), count (default: L; carry: 2 L - 1).  An integer may be given as
        a Python int or as a decimal or 0x string.  Raises KzgError(KZG_E_ARG) with the cause."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: wide: {why}")   # noqa: E731
        ops = list(ops) if isinstance(ops, (list, tuple)) else None
        if not ops or len(ops) > _native.KZG_WIDE_MAX_OPS:
            raise bad(f"ops must be a list of 1 .. {_native.KZG_WIDE_MAX_OPS} entries (n_ops)")
        is_u = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < top   # noqa: E731

        def big(v, name):
            if isinstance(v, str):
                try:
                    v = int(v, 0)
                except ValueError:
                    raise bad(f"{name} must be an integer, or a decimal or 0x string") from None
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise bad(f"{name} must be a non-negative integer")
            return v

        recs = []
        for op in ops:
            if not isinstance(op, dict) or "kind" not in op or "a" not in op:
                raise bad("an op is a mapping with kind, bits, limbs, a and the operands of its kind")
            extra = set(op) - set(cls._WIDE_KEYS)
            if extra:
                raise bad(f"unknown field {sorted(extra)[0]!r} (the fields are {', '.join(cls._WIDE_KEYS)})")
            name = op["kind"]
            if not isinstance(name, str) or name not in cls._WIDE_KINDS:
                raise bad(f"unknown kind {name!r} (one of {', '.join(cls._WIDE_KINDS)})")
            kind = cls._WIDE_KINDS[name]
            modular = name in ("mulmod", "carry")
            b, L = op.get("bits"), op.get("limbs")
            if not is_u(b, 65) or b == 0:
                raise bad("the limb width b (bits) must be an integer in [1, 64]")
            if not is_u(L, _native.KZG_WIDE_MAX_LIMBS + 1) or L == 0:
                raise bad(f"the number of limbs L (limbs) must be an integer in [1, {_native.KZG_WIDE_MAX_LIMBS}]")
            W = b * L
            if W > 512:
                raise bad("the width W = b L must be at most 512")
            if name == "carry" and b > 56:
                raise bad("the limb width b of a carry must be at most 56")
            counts = (2 * L - 1,) if name == "carry" else (L, L + 1) if name in ("add", "sub") else (L, 2 * L)
            count = op.get("count", counts[0])
            if not is_u(count, 17) or count not in counts:
                raise bad("count must be L or L + 1 on add and sub, L or 2 L on mul, divmod and mulmod, 2 L - 1 on carry")
            rows = {}
            for f in ("a", "b", "c", "q", "r"):
                v = op.get(f)
                if f == "b" and isinstance(v, (list, tuple)):
                    continue
                if v is None:
                    rows[f] = _native.KZG_WIDE_ABSENT
                elif is_u(v, _native.KZG_WIDE_ABSENT):
                    rows[f] = v
                else:
                    raise bad(f"operand {f} must be a first row, an integer in [0, 2^32 - 1), or None")
            if rows["a"] == _native.KZG_WIDE_ABSENT:
                raise bad("operand a must be given")
            flags, imm = 0, 0
            vb = op.get("b")
            if isinstance(vb, (list, tuple)):
                if len(vb) != 2 or vb[0] != "imm":
                    raise bad('an immediate is ("imm", value)')
                imm = big(vb[1], "an immediate")
                if imm >> W:
                    raise bad("the immediate must be below 2^W")
                flags |= _native.KZG_WIDE_IMM_B
                rows["b"] = _native.KZG_WIDE_ABSENT
            elif vb is None and not modular:
                raise bad("operand b must be given (a row or an immediate) on add, sub, mul and divmod")
            m = 0
            if modular:
                if op.get("m") is None:
                    raise bad("the modulus m must be given on mulmod and carry")
                m = big(op["m"], "the modulus m")
                if m == 0:
                    raise bad("the modulus m must not be 0")
                if m >> W:
                    raise bad("the modulus m must be below 2^W")
                if not isinstance(op.get("neg_c", False), bool):
                    raise bad("neg_c must be a boolean")
                if op.get("neg_c", False):
                    flags |= _native.KZG_WIDE_NEG_C
            elif op.get("c") is not None or op.get("m") is not None or op.get("neg_c"):
                raise bad(f"an operand the kind does not take: c, neg_c and m belong to mulmod and carry, not to {name}")
            if name == "carry":
                if op.get("q") is None or op.get("r") is None:
                    raise bad("operands q and r must be given on carry")
            elif op.get("q") is not None or op.get("r") is not None:
                raise bad(f"an operand the kind does not take: q and r belong to carry, not to {name}")
            recs.append((kind, b, L, count, flags, rows["a"], rows["b"], rows["c"], rows["q"], rows["r"],
                         imm.to_bytes(64, "big"), m.to_bytes(64, "big")))
        n_out = sum(r[3] for r in recs)
        if n_out > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"n_out: the ops give {n_out} output rows, at most {_native.KZG_MAX_BATCH_OPEN} fit one call")
        return recs

    @staticmethod
    def wide_op_struct(rec) -> "_native.WideOp":
        u8x64 = ctypes.c_uint8 * 64
        return _native.WideOp(*rec[:10], u8x64(*rec[10]), u8x64(*rec[11]))

    def commit_wide(self, input_sets: Sequence[object], ops: Sequence[dict], usable: Optional[int] = None,
                    tail: Sequence[bytes] = ()) -> Tuple["RowSet", dict]:
        """kzg_rows_commit_wide over the concatenated rows of input_sets (RowSet objects or bare handles).  ops: see wide_ops.
        A wide value is L consecutive rows, limb l in row first + l, each cell reduced to its low b bits.  The output rows of an
        op, in this order: add: L limbs of (a + b) mod 2^W, the carry; sub: L limbs of (a - b) mod 2^W, the borrow; mul: the low
        L limbs of a b, the high L limbs; divmod: L limbs of floor(a / b), L limbs of a mod b (2^W - 1 and a where b = 0);
        mulmod: with t = a b + d, L limbs of t mod m, L limbs of floor(t / m) (d = c, or m - (c mod m) with neg_c); carry: the
        2 L - 1 carry rows of the limb identity of that mulmod.  Returns (the new RowSet of all output rows in the order of ops;
        {"counts", "first", "qover", "first_qover"}: per op the rows with an out-of-range limb and the smallest such row or None,
        and the same for rows whose quotient passes 2^W (mulmod) or whose limb identity is inexact (carry)).  usable and tail:
        as for commit_int."""
        what = "commit_wide"
        ni, hi = self._handle_array(input_sets, what)
        recs = self.wide_ops(ops, what)
        n_out = sum(r[3] for r in recs)
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        arr = (_native.WideOp * len(recs))(*[self.wide_op_struct(r) for r in recs])
        c, h = ctypes.create_string_buffer(48 * n_out), ctypes.c_uint64(0)
        st = [(ctypes.c_uint64 * len(recs))() for _ in range(4)]
        self._chk(self._lib.kzg_rows_commit_wide(self._h, ni, hi, len(recs), arr, ctypes.byref(opts) if opts is not None else None,
                                                 c, st[0], st[1], st[2], st[3], ctypes.byref(h)))
        none = lambda vs: [None if int(v) == _native.KZG_INT_NONE else int(v) for v in vs]   # noqa: E731
        return (RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]),
                {"counts": [int(v) for v in st[0]], "first": none(st[1]), "qover": [int(v) for v in st[2]],
                 "first_qover": none(st[3])})

    # ---- a set built from sets: the Poseidon permutation (x^5, caller's constants) per row, as a check, or as a round trace
    _POSEIDON_PARAM_KEYS = ("t", "full", "partial", "rc", "mds")
    _POSEIDON_UNIT_KEYS = ("mode", "in", "out", "expect", "period")

    @classmethod
    def _poseidon_params(cls, params, sp):
        """The params of poseidon_call and poseidon_chain_call, checked and encoded by one body: (t, R, (t, full, partial, rc
        bytes, mds bytes)); sp: the caller's _UnitSpec"""
        bad = sp.bad
        if not isinstance(params, dict) or set(params) != set(cls._POSEIDON_PARAM_KEYS):
            raise bad(f"params is a mapping with exactly {', '.join(cls._POSEIDON_PARAM_KEYS)}")
        t, full, partial = params["t"], params["full"], params["partial"]
        if not _is_u(t, _native.KZG_POSEIDON_MAX_T + 1) or t < _native.KZG_POSEIDON_MIN_T:
            raise bad(f"the width t must be an integer in [{_native.KZG_POSEIDON_MIN_T}, {_native.KZG_POSEIDON_MAX_T}]")
        if not _is_u(full, _native.KZG_POSEIDON_MAX_FULL + 1) or full < 2 or full % 2:
            raise bad(f"the number of full rounds R_F must be even and in [2, {_native.KZG_POSEIDON_MAX_FULL}]")
        if not _is_u(partial, _native.KZG_POSEIDON_MAX_PARTIAL + 1):
            raise bad(f"the number of partial rounds R_P must be in [0, {_native.KZG_POSEIDON_MAX_PARTIAL}]")
        R = full + partial
        rc, mds = params["rc"], params["mds"]
        if not isinstance(rc, (list, tuple)) or len(rc) != t * R:
            raise bad(f"rc must be a list of t (R_F + R_P) = {t * R} scalars, round-major")
        if not isinstance(mds, (list, tuple)) or len(mds) != t * t:
            raise bad(f"mds must be a list of t t = {t * t} scalars, row-major")
        rc_b = b"".join(sp.scalar(v, "a round constant") for v in rc)
        mds_b = b"".join(sp.scalar(v, "a matrix entry") for v in mds)
        return t, R, (t, full, partial, rc_b, mds_b)

    @classmethod
    def poseidon_call(cls, params, units, what: str = "commit_poseidon") -> Tuple[tuple, List[tuple]]:
        """The kzg_poseidon_params fields (t, full, partial, rc bytes, mds bytes) and per unit the kzg_poseidon_unit fields
        (mode, flags, n_out, period, in[8], out[8], expect[8], imm[8] of 32 bytes) of a call.  params: a mapping with t (2 .. 8),
        full (R_F, even, 2 .. 16), partial (R_P, 0 .. 128), rc (t (R_F + R_P) scalars, round-major) and mds (t t scalars,
        row-major).  A unit is a mapping: mode "row" with in (t entries), out (1 .. t distinct state indices) and, for a check,
        expect (one row per entry of out); or mode "rounds" with in and period (at least R_F + R_P + 1).  An entry of in is a row
        index or ("imm", value).  A scalar is an int, a decimal or 0x string, or 32 big-endian bytes, below r.  Raises
        KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "poseidon")
        t, R, par = cls._poseidon_params(params, sp)
        return par, cls._poseidon_units(sp, t, R, 1, units)

    @classmethod
    def _poseidon_units(cls, sp, t: int, R: int, lead: int, units) -> List[tuple]:
        """The units of poseidon_call and poseidon2_call, parsed by one body into kzg_poseidon_unit fields; a trace block holds
        R + lead rows (lead = 1: Poseidon; 2: Poseidon2, with its row of E(input)); sp: the caller's _UnitSpec"""
        bad = sp.bad
        recs = []
        for un in sp.units(units, _native.KZG_POSEIDON_MAX_UNITS):
            if not isinstance(un, dict) or "mode" not in un or "in" not in un:
                raise bad("a unit is a mapping with mode, in and the fields of its mode")
            extra = set(un) - set(cls._POSEIDON_UNIT_KEYS)
            if extra:
                raise bad(f"unknown field {sorted(extra)[0]!r} (the fields are {', '.join(cls._POSEIDON_UNIT_KEYS)})")
            mode = un["mode"]
            if mode not in ("row", "rounds"):
                raise bad(f'unknown mode {mode!r} (one of "row", "rounds")')
            rows, imms = sp.slots(un["in"], t, lambda: f'in must hold t = {t} entries, each a row index or ("imm", value)',
                                  "an entry of in")
            flags, period, expect = 0, 0, []
            if mode == "rounds":
                if un.get("expect") is not None:
                    raise bad("expect belongs to row units, not to rounds")
                if un.get("out") is not None:
                    raise bad("out belongs to row units: a rounds unit commits all t columns")
                period = sp.period(un.get("period"), R + lead, lambda: "the period P of a rounds unit must be an integer in "
                                   f"[R + {lead}, 2^32), R + {lead} = {R + lead}")
                out = list(range(t))
            else:
                if un.get("period") is not None:
                    raise bad("period belongs to rounds units, not to row")
                out = sp.indices(un.get("out"), t, t, lambda: f"out must hold 1 .. t = {t} state indices",
                                 lambda: f"an out index must be an integer below t = {t}", "an out index is repeated")
                if un.get("expect") is not None:
                    expect, flags = sp.expects(un["expect"], len(out)), _native.KZG_POSEIDON_CHECK
            recs.append((_native.KZG_POSEIDON_ROW if mode == "row" else _native.KZG_POSEIDON_ROUNDS, flags, len(out), period,
                         _pad(rows, 8), _pad(out, 8), _pad(expect, 8), _pad(imms, 8, _ZERO32)))
        sp.caps(sum(r[2] for r in recs if not r[1]))
        return recs

    @staticmethod
    def poseidon_unit_struct(rec) -> "_native.PoseidonUnit":
        u = _native.PoseidonUnit(rec[0], rec[1], rec[2], rec[3], (ctypes.c_uint32 * 8)(*rec[4]), (ctypes.c_uint32 * 8)(*rec[5]),
                                 (ctypes.c_uint32 * 8)(*rec[6]))
        for j, b in enumerate(rec[7]):
            u.imm_be32[j][:] = list(b)
        return u

    def commit_poseidon(self, input_sets: Sequence[object], params: dict, units: Sequence[dict], usable: Optional[int] = None,
                        tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_poseidon over the concatenated rows of input_sets (RowSet objects or bare handles).  params and units:
        see poseidon_call.  The permutation is the plain Hades schedule with the S-box x^5: per round s_i += rc[rho t + i]; s_i
        <- s_i^5 for every i in a full round, for i = 0 in a partial one; s <- M s.  A row unit hashes every row t' < n (n =
        usable, or T) and commits one column per entry of out -- or, with expect, commits nothing and counts the rows whose
        expected cells differ; a rounds unit commits the t columns of the round trace, one block of `period` rows per
        permutation.  Returns (the new RowSet of all committed columns in unit order, or None when every unit is a check;
        {"perms", "mismatch", "first_mismatch"} per unit).  usable and tail: as for commit_derived, the tail column-major over
        the committed columns."""
        what = "commit_poseidon"
        ni, hi = self._handle_array(input_sets, what)
        par, recs = self.poseidon_call(params, units, what)
        arr = (_native.PoseidonUnit * len(recs))(*[self.poseidon_unit_struct(r) for r in recs])
        return self._commit_units(what, self._lib.kzg_rows_commit_poseidon, input_sets, ni, hi, _native.PoseidonParams(*par), arr,
                                  sum(r[2] for r in recs if not r[1]), usable, tail,
                                  (("perms", 0), ("mismatch", 0), ("first_mismatch", 1)), _native.KZG_POSEIDON_NONE)

    # ---- a set built from sets: the Poseidon2 permutation (product-free external layer), the units of commit_poseidon
    _POSEIDON2_PARAM_KEYS = ("t", "full", "partial", "rc_full", "rc_partial", "diag")
    _POSEIDON2_WIDTHS = tuple(t for t in range(32) if _native.KZG_POSEIDON2_WIDTHS >> t & 1)

    @classmethod
    def poseidon2_call(cls, params, units, what: str = "commit_poseidon2") -> Tuple[tuple, List[tuple]]:
        """The kzg_poseidon2_params fields (t, full, partial, rc_full bytes, rc_partial bytes, diag bytes) and per unit the
        kzg_poseidon_unit fields as poseidon_call returns them (from the same body).  params: a mapping with t (2, 3, 4 or 8),
        full (R_F, even, 2 .. 16), partial (R_P, 0 .. 128), rc_full (t R_F scalars, round-major over the full rounds of both
        halves), rc_partial (R_P scalars) and diag (t scalars: the internal layer is the all-ones matrix plus diag).  Units: as
        for poseidon_call, with a period of at least R_F + R_P + 2.  Raises KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "poseidon2")
        bad = sp.bad
        if not isinstance(params, dict) or set(params) != set(cls._POSEIDON2_PARAM_KEYS):
            raise bad(f"params is a mapping with exactly {', '.join(cls._POSEIDON2_PARAM_KEYS)}")
        t, full, partial = params["t"], params["full"], params["partial"]
        if not _is_u(t, 32) or t not in cls._POSEIDON2_WIDTHS:
            raise bad(f"the width t must be one of {', '.join(map(str, cls._POSEIDON2_WIDTHS))}")
        if not _is_u(full, _native.KZG_POSEIDON2_MAX_FULL + 1) or full < 2 or full % 2:
            raise bad(f"the number of full rounds R_F must be even and in [2, {_native.KZG_POSEIDON2_MAX_FULL}]")
        if not _is_u(partial, _native.KZG_POSEIDON2_MAX_PARTIAL + 1):
            raise bad(f"the number of partial rounds R_P must be in [0, {_native.KZG_POSEIDON2_MAX_PARTIAL}]")
        lists = []
        for name, count, words, kind in (("rc_full", t * full, "t R_F", "a round constant"),
                                         ("rc_partial", partial, "R_P", "a round constant"), ("diag", t, "t", "a diagonal entry")):
            v = params[name]
            if not isinstance(v, (list, tuple)) or len(v) != count:
                raise bad(f"{name} must be a list of {words} = {count} scalars")
            lists.append(b"".join(sp.scalar(x, kind) for x in v))
        return (t, full, partial, *lists), cls._poseidon_units(sp, t, full + partial, 2, units)

    def commit_poseidon2(self, input_sets: Sequence[object], params: dict, units: Sequence[dict], usable: Optional[int] = None,
                         tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_poseidon2 over the concatenated rows of input_sets: commit_poseidon with the Poseidon2 permutation.
        params and units: see poseidon2_call.  s <- E(s); R_F / 2 full rounds (s_i += rc_full[..]; s_i <- s_i^5; s <- E(s)); R_P
        partial rounds (s_0 += rc_partial[rho]; s_0 <- s_0^5; s <- I(s)); R_F / 2 full rounds.  A rounds unit's block holds the
        input, E(input), then the state behind every round: R + 2 rows.  Returns what commit_poseidon returns."""
        what = "commit_poseidon2"
        ni, hi = self._handle_array(input_sets, what)
        par, recs = self.poseidon2_call(params, units, what)
        arr = (_native.PoseidonUnit * len(recs))(*[self.poseidon_unit_struct(r) for r in recs])
        return self._commit_units(what, self._lib.kzg_rows_commit_poseidon2, input_sets, ni, hi, _native.Poseidon2Params(*par),
                                  arr, sum(r[2] for r in recs if not r[1]), usable, tail,
                                  (("perms", 0), ("mismatch", 0), ("first_mismatch", 1)), _native.KZG_POSEIDON_NONE)

    def _commit_units(self, what, fn, input_sets, ni, hi, lead, arr, n_out, usable, tail, stats, none):
        """The one body behind the seven unit builders' commit_*, from the layout on (fn: the library's call; ni, hi: the handle
        array; lead: the params or curve struct in front of the unit array `arr`, None where the builder has none).  stats: a
        (name, is a first row) pair per statistics array in the call's order; `none` in a first-row array becomes None.
        Returns (the new RowSet or None when nothing is committed, {name: one value per unit})."""
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        c, h = ctypes.create_string_buffer(48 * max(n_out, 1)), ctypes.c_uint64(0)
        st = [(ctypes.c_uint64 * len(arr))() for _ in stats]
        front = (self._h, ni, hi) if lead is None else (self._h, ni, hi, ctypes.byref(lead))
        self._chk(fn(*front, len(arr), arr, ctypes.byref(opts) if opts is not None else None, c if n_out else None, *st,
                     ctypes.byref(h)))
        rs = RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]) if n_out else None
        return rs, {name: [None if v == none else v for v in xs] if first else list(xs) for (name, first), xs in zip(stats, st)}

    @staticmethod
    def _n_rows(input_sets):
        """the number of concatenated input rows where every set says its own (a RowSet does, a bare handle does not)"""
        ks = [getattr(x, "k", None) for x in input_sets]
        return None if any(k is None for k in ks) else sum(ks)

    # ---- a set built from sets: Poseidon sponges and Merkle paths, chained from block to block along the column
    _POSEIDON_CHAIN_KEYS = {"sponge": ("mode", "in", "start", "period", "layout", "cols", "digest", "expect"),
                            "path": ("mode", "cap", "leaf", "sib", "pos", "digest", "start", "period", "layout", "cols", "expect")}

    @classmethod
    def poseidon_chain_call(cls, params, units, what: str = "commit_poseidon_chain") -> Tuple[tuple, List[tuple]]:
        """The kzg_poseidon_params fields (as poseidon_call returns them, from the same body) and per unit the
        kzg_poseidon_chain_unit fields (mode, flags, layout, period, start, pos, digest, expect, n_out, in[8], out[16], imm[8] of 32
        bytes) of a call.  A unit is a mapping.  {"mode": "sponge", "in": t slots, "start": row or None, "period": P, "layout":
        "trace" or "flat"}; {"mode": "path", "cap": slot, "leaf": slot, "sib": t - 2 rows, "pos": row, "digest": j, "start": row or
        None, "period": P, "layout": ...}.  "flat" takes "cols": 1 .. 2 t distinct names among in0 .. in{t-1}, out0 .. out{t-1};
        "trace" needs P >= R_F + R_P + 1.  Either mode with "expect": row (and "digest") in place of layout and cols is a check.
        A slot is a row index or ("imm", value).  Raises KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "poseidon_chain")
        bad = sp.bad
        t, R, par = cls._poseidon_params(params, sp)
        ABSENT = _native.KZG_POSEIDON_CHAIN_ABSENT
        recs = []

        def row(v, name, optional=False):
            if v is None and optional:
                return ABSENT
            if isinstance(v, (list, tuple)):
                raise bad(f"{name} must be a row, not an immediate")
            return sp.row(v, lambda: f"{name} must be a row index, an integer in [0, 2^32 - 1)")

        for un in sp.units(units, _native.KZG_POSEIDON_CHAIN_MAX_UNITS):
            mode = sp.mode(un, cls._POSEIDON_CHAIN_KEYS, foreign=True)
            if mode == "sponge":
                rows, imms = sp.slots(un.get("in"), t, lambda: f'in must hold t = {t} entries, each a row index or ("imm", value)',
                                      "an entry of in")
                pos = ABSENT
            else:
                if t < 3:
                    raise bad("a path unit needs t >= 3: the arity is t - 1")
                if "cap" not in un or "leaf" not in un:
                    raise bad("a path unit needs cap and leaf, each a row index or (\"imm\", value)")
                sib = un.get("sib")
                if not isinstance(sib, (list, tuple)) or len(sib) != t - 2:
                    raise bad(f"sib must hold t - 2 = {t - 2} rows")
                (cap, cap_imm), (leaf, leaf_imm) = sp.slot(un["cap"], "cap"), sp.slot(un["leaf"], "leaf")
                rows, imms = [cap, leaf] + [row(v, "an entry of sib") for v in sib], [cap_imm, leaf_imm] + [_ZERO32] * (t - 2)
                pos = row(un.get("pos"), "pos")
            start = row(un.get("start"), "start", optional=True)
            period = sp.period(un.get("period"), 1, "the period P must be an integer in [1, 2^32)")
            digest = un.get("digest")
            if digest is not None and not _is_u(digest, t):
                raise bad(f"digest must be a state index below t = {t}")
            flags, layout, out, expect = 0, 0, [], ABSENT
            if un.get("expect") is not None:
                if un.get("layout") is not None or un.get("cols") is not None:
                    raise bad("layout and cols are refused beside expect: a check commits nothing")
                if digest is None:
                    raise bad("expect needs digest, the state index that is compared")
                expect = row(un["expect"], "expect")
                flags = _native.KZG_POSEIDON_CHAIN_CHECK
            else:
                if mode == "path" and digest is None:
                    raise bad("a path unit needs digest, the state index that a continuing block hashes")
                if mode == "sponge" and digest is not None:
                    raise bad("digest belongs to path units and to checks (expect)")
                lay = un.get("layout")
                if lay not in ("trace", "flat"):
                    raise bad(f'unknown layout {lay!r} (one of "trace", "flat")')
                if lay == "trace":
                    if un.get("cols") is not None:
                        raise bad("cols belongs to the flat layout: a trace commits all t columns")
                    if period < R + 1:
                        raise bad(f"the period P of a trace must be at least R + 1 = {R + 1}")
                    layout, out = _native.KZG_POSEIDON_CHAIN_TRACE, list(range(t))
                else:
                    names = [f"in{j}" for j in range(t)] + [f"out{j}" for j in range(t)]
                    ids = [_native.KZG_POSEIDON_CHAIN_COL_IN + j for j in range(t)] + \
                          [_native.KZG_POSEIDON_CHAIN_COL_OUT + j for j in range(t)]
                    picked = sp.names(un.get("cols"), names,
                                      lambda: f"cols must hold 1 .. 2 t = {2 * t} column names among {', '.join(names)}")
                    layout, out = _native.KZG_POSEIDON_CHAIN_FLAT, [ids[k] for k in picked]
            recs.append((_native.KZG_POSEIDON_CHAIN_SPONGE if mode == "sponge" else _native.KZG_POSEIDON_CHAIN_PATH, flags, layout,
                         period, start, pos, ABSENT if digest is None else digest, expect, len(out),
                         _pad(rows, 8), _pad(out, 16), _pad(imms, 8, _ZERO32)))
        sp.caps(sum(r[8] for r in recs))
        return par, recs

    @staticmethod
    def poseidon_chain_unit_struct(rec) -> "_native.PoseidonChainUnit":
        u = _native.PoseidonChainUnit(*rec[:9], 0, (ctypes.c_uint32 * 8)(*rec[9]), (ctypes.c_uint32 * 16)(*rec[10]))
        for j, b in enumerate(rec[11]):
            u.imm_be32[j][:] = list(b)
        return u

    def commit_poseidon_chain(self, input_sets: Sequence[object], params: dict, units: Sequence[dict],
                              usable: Optional[int] = None, tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_poseidon_chain over the concatenated rows of input_sets (RowSet objects or bare handles).  params: as
        for commit_poseidon; units: see poseidon_chain_call.  Every unit is a chain over blocks of `period` rows, b < floor(n /
        P) with n = usable, or T: block b starts a segment when b = 0, start is None or its start cell at row b P is not zero,
        and continues the block before otherwise.  A sponge block that continues adds its cells to the output before it (an
        immediate enters once per segment); a path block hashes cap and the t - 1 children, the child at position pos being the
        leaf (a starting block) or element digest of the output before (a pos cell at or above t - 1 is position 0 and counted).
        Layout "trace" commits the t columns of the round trace, "flat" the named in / out columns at the block's first row;
        with expect the unit commits nothing and compares element digest of every segment's last output.  A segment is serial:
        one lane walks it.  Returns (the new RowSet of all committed columns in unit order, or None when every unit is a check;
        {"blocks", "segments", "bad_pos", "first_bad_pos", "mismatch", "first_mismatch"} per unit).  usable and tail: as for
        commit_poseidon."""
        what = "commit_poseidon_chain"
        ni, hi = self._handle_array(input_sets, what)
        par, recs = self.poseidon_chain_call(params, units, what)
        arr = (_native.PoseidonChainUnit * len(recs))(*[self.poseidon_chain_unit_struct(r) for r in recs])
        return self._commit_units(what, self._lib.kzg_rows_commit_poseidon_chain, input_sets, ni, hi,
                                  _native.PoseidonParams(*par), arr, sum(r[8] for r in recs), usable, tail,
                                  (("blocks", 0), ("segments", 0), ("bad_pos", 0), ("first_bad_pos", 1), ("mismatch", 0),
                                   ("first_mismatch", 1)), _native.KZG_POSEIDON_NONE)

    # ---- a set built from sets: the SHA-256 compression per row, as a check, or as a chained round trace
    _SHA256_KEYS = {"row": ("mode", "state", "msg", "out", "expect"), "rounds": ("mode", "msg", "start", "period", "iv", "cols")}

    @classmethod
    def sha256_call(cls, units, what: str = "commit_sha256") -> List[tuple]:
        """Per unit the kzg_sha256_unit fields (mode, flags, n_out, period, start, state[8], state_imm[8], msg[16], msg_imm[16],
        out[12], expect[8]) of a call.  A unit is a mapping.  {"mode": "row", "state": "iv" or 8 slots, "msg": 16 slots, "out":
        1 .. 8 distinct word indices below 8} and, for a check, "expect": one row per entry of out.  {"mode": "rounds", "msg":
        row, "start": row or None, "period": P >= 72, "iv": None or 8 words, "cols": 1 .. 12 distinct names of
        _native.KZG_SHA256_COLS}.  A slot is a row index or ("imm", v) with v < 2^32.  Raises KzgError(KZG_E_ARG) with the
        cause; needs no device."""
        sp = _UnitSpec(what, "sha256")
        bad = sp.bad
        IMM = _native.KZG_SHA256_IMM

        def slots(v, count, name):
            return sp.slots(v, count, lambda: f'{name} must hold {count} slots, each a row index or ("imm", value)', "a slot", 32)

        recs = []
        for un in sp.units(units, _native.KZG_SHA256_MAX_UNITS):
            mode = sp.mode(un, cls._SHA256_KEYS, "expect belongs to row units, not to rounds")
            flags, period, start, expect = 0, 0, _native.KZG_SHA256_ABSENT, []
            if mode == "row":
                state = un.get("state")
                if state == "iv":
                    flags |= _native.KZG_SHA256_STD_IV
                    st_rows, st_imm = [IMM] * 8, [0] * 8
                else:
                    st_rows, st_imm = slots(state, 8, 'state ("iv", or a list)')
                m_rows, m_imm = slots(un.get("msg"), 16, "msg")
                out = sp.indices(un.get("out"), 8, 8, "out must hold 1 .. 8 word indices", "an out index must be an integer below 8",
                                 "an out index is repeated")
                if un.get("expect") is not None:
                    expect = sp.expects(un["expect"], len(out))
                    flags |= _native.KZG_SHA256_CHECK
            else:
                msg = sp.row(un.get("msg"), "the msg of a rounds unit must be a row index, an integer in [0, 2^32 - 1)")
                m_rows, m_imm = [msg] + [0] * 15, [0] * 16
                if un.get("start") is not None:
                    start = sp.row(un["start"], "start must be a row index, an integer in [0, 2^32 - 1), or None")
                period = sp.period(un.get("period"), _native.KZG_SHA256_MIN_PERIOD,
                                   lambda: f"the period P of a rounds unit must be an integer in [{_native.KZG_SHA256_MIN_PERIOD}, 2^32)")
                st_rows = [IMM] * 8
                if un.get("iv") is None:
                    flags |= _native.KZG_SHA256_STD_IV
                    st_imm = [0] * 8
                else:
                    st_imm = un["iv"]
                    if not isinstance(st_imm, (list, tuple)) or len(st_imm) != 8 or any(not _is_u(v, 1 << 32) for v in st_imm):
                        raise bad("iv must be None or 8 words, integers below 2^32")
                    st_imm = list(st_imm)
                out = sp.names(un.get("cols"), _native.KZG_SHA256_COLS, lambda: f"cols must hold 1 .. {_native.KZG_SHA256_N_COLS} column names")
            recs.append((_native.KZG_SHA256_ROW if mode == "row" else _native.KZG_SHA256_ROUNDS, flags, len(out), period, start,
                         st_rows, st_imm, m_rows, m_imm, _pad(out, 12), _pad(expect, 8)))
        sp.caps(sum(r[2] for r in recs if not r[1] & _native.KZG_SHA256_CHECK))
        return recs

    @staticmethod
    def sha256_unit_struct(rec) -> "_native.Sha256Unit":
        A = lambda k, xs: (ctypes.c_uint32 * k)(*xs)   # noqa: E731
        return _native.Sha256Unit(rec[0], rec[1], rec[2], rec[3], rec[4], A(8, rec[5]), A(8, rec[6]), A(16, rec[7]), A(16, rec[8]),
                                  A(12, rec[9]), A(8, rec[10]))

    _HASH_STATS = (("messages", 0), ("counts", 0), ("first", 1), ("mismatch", 0), ("first_mismatch", 1))

    def commit_sha256(self, input_sets: Sequence[object], units: Sequence[dict], usable: Optional[int] = None,
                      tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_sha256 over the concatenated rows of input_sets (RowSet objects or bare handles).  units: see
        sha256_call.  All values are 32-bit words: a source cell is its canonical integer reduced to its low 32 bits, and a
        cell at or above 2^32 is counted.  A row unit runs one compression per row t' < n (n = usable, or T) and commits one
        column per entry of out -- or, with expect, commits nothing and counts the rows whose expected cells differ; a rounds
        unit commits the named columns of the round trace in blocks of `period` rows, chained along the start column.
        Returns (the new RowSet of all committed columns in unit order, or None when every unit is a check; {"blocks",
        "messages", "counts", "first", "mismatch", "first_mismatch"} per unit).  usable and tail: as for commit_derived, the
        tail column-major over the committed columns."""
        what = "commit_sha256"
        ni, hi = self._handle_array(input_sets, what)
        recs = self.sha256_call(units, what)
        arr = (_native.Sha256Unit * len(recs))(*[self.sha256_unit_struct(r) for r in recs])
        return self._commit_units(what, self._lib.kzg_rows_commit_sha256, input_sets, ni, hi, None, arr,
                                  sum(r[2] for r in recs if not r[1] & _native.KZG_SHA256_CHECK), usable, tail,
                                  (("blocks", 0),) + self._HASH_STATS, _native.KZG_SHA256_NONE)

    # ---- a set built from sets: Keccak-f[1600] per row, as a check, or as a chained round trace of 64-bit lanes
    _KECCAK_KEYS = {"row": ("mode", "in", "out", "expect"), "rounds": ("mode", "msg", "rate", "start", "period", "cols")}

    @classmethod
    def keccak_call(cls, units, what: str = "commit_keccak") -> List[tuple]:
        """Per unit the kzg_keccak_unit fields (mode, flags, n_out, period, rate, start, imm[25], in[25], out[16], expect[16])
        of a call.  A unit is a mapping.  {"mode": "row", "in": 25 slots, "out": 1 .. 16 distinct lane indices below 25} and,
        for a check, "expect": one row per entry of out.  {"mode": "rounds", "msg": 5 rows, "rate": 1 .. 24, "start": row or
        None, "period": P >= 125, "cols": 1 .. 16 distinct names of _native.KZG_KECCAK_COLS}.  A slot is a row index or ("imm",
        v) with v < 2^64; lane (x, y) is slot x + 5 y.  Raises KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "keccak")
        bad = sp.bad
        IMM, TOP = _native.KZG_KECCAK_IMM, _native.KZG_KECCAK_MAX_OUT
        recs = []
        for un in sp.units(units, _native.KZG_KECCAK_MAX_UNITS):
            mode = sp.mode(un, cls._KECCAK_KEYS, "expect belongs to row units, not to rounds")
            flags, period, rate, start, expect = 0, 0, 0, _native.KZG_KECCAK_ABSENT, []
            if mode == "row":
                rows, imms = sp.slots(un.get("in"), 25, 'in must hold 25 slots, each a row index or ("imm", value)', "a slot", 64)
                out = sp.indices(un.get("out"), TOP, 25, lambda: f"out must hold 1 .. {TOP} lane indices (n_out)",
                                 "a lane index must be an integer below 25", "a lane index is repeated")
                if un.get("expect") is not None:
                    expect = sp.expects(un["expect"], len(out))
                    flags |= _native.KZG_KECCAK_CHECK
            else:
                msg = un.get("msg")
                if not isinstance(msg, (list, tuple)) or len(msg) != 5 or any(not _is_u(r, IMM) for r in msg):
                    raise bad("the msg of a rounds unit must hold 5 row indices, integers in [0, 2^32 - 1)")
                sp.seen.update(msg)
                rows, imms = list(msg) + [0] * 20, [0] * 25
                rate = un.get("rate")
                if not _is_u(rate, 25) or rate < 1:
                    raise bad("the rate of a rounds unit must be an integer in [1, 24] lanes")
                if un.get("start") is not None:
                    start = sp.row(un["start"], "start must be a row index, an integer in [0, 2^32 - 1), or None")
                period = sp.period(un.get("period"), _native.KZG_KECCAK_MIN_PERIOD,
                                   lambda: f"the period P of a rounds unit must be an integer in [{_native.KZG_KECCAK_MIN_PERIOD}, 2^32)")
                out = sp.names(un.get("cols"), _native.KZG_KECCAK_COLS, lambda: f"cols must hold 1 .. {TOP} column names (n_out)", top=TOP)
            recs.append((_native.KZG_KECCAK_ROW if mode == "row" else _native.KZG_KECCAK_ROUNDS, flags, len(out), period, rate,
                         start, imms, rows, _pad(out, 16), _pad(expect, 16)))
        sp.caps(sum(r[2] for r in recs if not r[1] & _native.KZG_KECCAK_CHECK))
        return recs

    @staticmethod
    def keccak_unit_struct(rec) -> "_native.KeccakUnit":
        A = lambda k, xs: (ctypes.c_uint32 * k)(*xs)   # noqa: E731
        return _native.KeccakUnit(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], (ctypes.c_uint64 * 25)(*rec[6]), A(25, rec[7]),
                                  A(16, rec[8]), A(16, rec[9]))

    def commit_keccak(self, input_sets: Sequence[object], units: Sequence[dict], usable: Optional[int] = None,
                      tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_keccak over the concatenated rows of input_sets (RowSet objects or bare handles).  units: see
        keccak_call.  All values are 64-bit lanes: a source cell is its canonical integer reduced to its low 64 bits, and a
        cell at or above 2^64 is counted.  A row unit runs one Keccak-f[1600] per row t' < n (n = usable, or T) and commits one
        column per entry of out -- or, with expect, commits nothing and counts the rows whose expected cells differ; a rounds
        unit commits the named columns of the round trace in blocks of `period` rows, chained along the start column.
        Returns (the new RowSet of all committed columns in unit order, or None when every unit is a check; {"perms",
        "messages", "counts", "first", "mismatch", "first_mismatch"} per unit).  usable and tail: as for commit_derived, the
        tail column-major over the committed columns."""
        what = "commit_keccak"
        ni, hi = self._handle_array(input_sets, what)
        recs = self.keccak_call(units, what)
        arr = (_native.KeccakUnit * len(recs))(*[self.keccak_unit_struct(r) for r in recs])
        return self._commit_units(what, self._lib.kzg_rows_commit_keccak, input_sets, ni, hi, None, arr,
                                  sum(r[2] for r in recs if not r[1] & _native.KZG_KECCAK_CHECK), usable, tail,
                                  (("perms", 0),) + self._HASH_STATS, _native.KZG_KECCAK_NONE)

    # ---- a set built from sets: arithmetic of an elliptic curve over a foreign field: a / b mod p, point addition, chains
    _EC_CURVE_KEYS = ("bits", "limbs", "p", "a")
    _EC_KEYS = {"div": ("mode", "a", "b", "out", "expect"), "add": ("mode", "x1", "y1", "x2", "y2", "out", "expect"),
                "chain": ("mode", "px", "py", "op", "cols")}
    _EC_MODES = {"div": _native.KZG_EC_DIV, "add": _native.KZG_EC_ADD, "chain": _native.KZG_EC_CHAIN}

    @classmethod
    def ec_call(cls, curve, units, what: str = "commit_ec", n_rows: Optional[int] = None) -> Tuple[tuple, List[tuple]]:
        """The kzg_ec_curve fields (bits, limbs, p, a) and per unit the kzg_ec_unit fields (mode, flags, cols, op, in[4],
        expect[3], imm) of a call.  curve: a mapping with bits (b in [1, 64]), limbs (L in [1, 4], W = b L <= 256), p (odd, 3 <=
        p < 2^W) and a (below p).  A unit is a mapping.  {"mode": "div", "a": first row, "b": first row or ("imm", v), "out":
        True}; {"mode": "add", "x1", "y1", "x2", "y2": first rows, "out": names among lam, x3, y3}; either with "expect" in
        place of out is a check: one first row for div, three entries for add (lam, x3, y3; None: that name is not compared).
        {"mode": "chain", "px", "py": first rows, "op": row, "cols": names among ax, ay, lam}.  An integer may be given as a
        Python int or as a decimal or 0x string.  n_rows: the number of concatenated input rows, where known: an operand run
        must lie inside.  Raises KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "ec")
        bad = sp.bad
        ABSENT = _native.KZG_EC_ABSENT

        def big(v, name):
            if isinstance(v, str):
                try:
                    v = int(v, 0)
                except ValueError:
                    raise bad(f"{name} must be an integer, or a decimal or 0x string") from None
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise bad(f"{name} must be a non-negative integer")
            return v

        if not isinstance(curve, dict):
            raise bad("the curve is a mapping with bits, limbs, p and a")
        extra = set(curve) - set(cls._EC_CURVE_KEYS)
        if extra:
            raise bad(f"unknown field {sorted(extra)[0]!r} of the curve (the fields are {', '.join(cls._EC_CURVE_KEYS)})")
        b, L = curve.get("bits"), curve.get("limbs")
        if not _is_u(b, 65) or b == 0:
            raise bad("the limb width b (bits) must be an integer in [1, 64]")
        if not _is_u(L, _native.KZG_EC_MAX_LIMBS + 1) or L == 0:
            raise bad(f"the number of limbs L (limbs) must be an integer in [1, {_native.KZG_EC_MAX_LIMBS}]")
        W = b * L
        if W > 256:
            raise bad("the width W = b L must be at most 256")
        if curve.get("p") is None or curve.get("a") is None:
            raise bad("the curve must give the modulus p and the coefficient a")
        p, a = big(curve["p"], "the modulus p"), big(curve["a"], "the coefficient a")
        if p % 2 == 0 or p < 3:
            raise bad("the modulus p must be odd and at least 3")
        if p >> W:
            raise bad("the modulus p must be below 2^W")
        if a >= p:
            raise bad("the coefficient a must be below p")
        recs, n_out = [], 0

        def run(v, name, count=L):
            if not _is_u(v, ABSENT):
                raise bad(f"{name} must be a first row, an integer in [0, 2^32 - 1)")
            if n_rows is not None and v + count > n_rows:
                raise bad(f"the operand run of {name} reaches beyond the {n_rows} concatenated rows of the input sets")
            sp.seen.update(range(v, v + count))
            return v

        for un in sp.units(units, _native.KZG_EC_MAX_UNITS):
            mode = sp.mode(un, cls._EC_KEYS, "expect belongs to div and add units, not to chain")
            flags, op, imm, ins, expect = 0, ABSENT, 0, [ABSENT] * 4, [ABSENT] * 3
            if mode == "chain":
                ins[0], ins[1] = run(un.get("px"), "px"), run(un.get("py"), "py")
                op = run(un.get("op"), "op", 1)
                names = _native.KZG_EC_CHAIN_NAMES
                picked = sp.names(un.get("cols"), names, lambda: f"cols must hold 1 .. 3 column names among {', '.join(names)}", "name", mode)
            else:
                names = ("r",) if mode == "div" else _native.KZG_EC_ADD_NAMES
                if mode == "div":
                    ins[0] = run(un.get("a"), "a")
                    vb = un.get("b")
                    if isinstance(vb, (list, tuple)):
                        if len(vb) != 2 or vb[0] != "imm":
                            raise bad('an immediate is ("imm", value)')
                        imm = big(vb[1], "an immediate")
                        if imm >> W:
                            raise bad("the immediate must be below 2^W")
                        flags |= _native.KZG_EC_IMM_B
                    else:
                        ins[1] = run(vb, "b")
                else:
                    ins = [run(un.get(k), k) for k in ("x1", "y1", "x2", "y2")]
                if sp.out_or_expect(un):
                    ex = un["expect"]
                    if not isinstance(ex, (list, tuple)) or len(ex) != len(names):
                        raise bad("a wrong number of expect rows: one first row for div, three entries (lam, x3, y3; None: not "
                                  "compared) for add")
                    picked = [j for j, v in enumerate(ex) if v is not None]
                    if not picked:
                        raise bad("expect must name at least one first row")
                    for j in picked:
                        expect[j] = run(ex[j], "an entry of expect")
                    flags |= _native.KZG_EC_CHECK
                elif mode == "div":
                    if un["out"] is not True:
                        raise bad("the out of a div unit is True")
                    picked = [0]
                else:
                    picked = sp.names(un["out"], names, lambda: f"out must hold 1 .. 3 names among {', '.join(names)}", "name", mode)
            if not flags & _native.KZG_EC_CHECK:
                n_out += len(picked) * L
            recs.append((cls._EC_MODES[mode], flags, sum(1 << k for k in picked), op, ins, expect, imm))
        sp.caps(n_out)
        return (b, L, p, a), recs

    @staticmethod
    def ec_structs(cv, recs) -> Tuple["_native.EcCurve", object]:
        w64 = lambda v: (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & 0xffffffffffffffff for k in range(4)])   # noqa: E731
        curve = _native.EcCurve(cv[0], cv[1], w64(cv[2]), w64(cv[3]))
        arr = (_native.EcUnit * len(recs))(*[_native.EcUnit(r[0], r[1], r[2], r[3], (ctypes.c_uint32 * 4)(*r[4]),
                                                            (ctypes.c_uint32 * 3)(*r[5]), 0, w64(r[6])) for r in recs])
        return curve, arr

    @staticmethod
    def ec_n_out(cv, recs) -> int:
        return sum(bin(r[2]).count("1") * cv[1] for r in recs if not r[1] & _native.KZG_EC_CHECK)

    _CURVE_STATS = (("singular", 0), ("first_singular", 1), ("mismatch", 0), ("first_mismatch", 1), ("unknown", 0),
                    ("first_unknown", 1), ("segments", 0))

    def commit_ec(self, input_sets: Sequence[object], curve: dict, units: Sequence[dict], usable: Optional[int] = None,
                  tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_ec over the concatenated rows of input_sets (RowSet objects or bare handles).  curve and units: see
        ec_call.  A wide value is L consecutive rows of b bits; an operand at or above p is reduced mod p and its row counted.
        A div unit commits the L rows of a b^-1 mod p (0 and `singular` where b has no inverse); an add unit the named ones of
        lam, x3, y3 of (x1, y1) + (x2, y2), the doubling where the points are equal, zeros and `singular` on an exceptional
        row; either with expect commits nothing and counts the rows whose expected cells differ; a chain unit commits the named
        ones of ax, ay, lam: the accumulator before each row's step and the step's lambda, for the op-codes 0 hold, 1 load, 2
        add (px, py), 3 double.  Returns (the new RowSet of all committed rows in unit order, or None when every unit is a
        check; {"counts", "first", "singular", "first_singular", "mismatch", "first_mismatch", "unknown", "first_unknown",
        "segments"} per unit).  usable and tail: as for commit_derived, the tail column-major over the committed rows."""
        what = "commit_ec"
        ni, hi = self._handle_array(input_sets, what)
        cv, recs = self.ec_call(curve, units, what, self._n_rows(input_sets))
        cs, arr = self.ec_structs(cv, recs)
        return self._commit_units(what, self._lib.kzg_rows_commit_ec, input_sets, ni, hi, cs, arr, self.ec_n_out(cv, recs), usable,
                                  tail, (("counts", 0), ("first", 1)) + self._CURVE_STATS, _native.KZG_EC_NONE)

    # ---- a set built from sets: arithmetic of a twisted Edwards curve over the scalar field itself: point addition, chains
    _EDWARDS_CURVE_KEYS = ("a", "d")
    _EDWARDS_KEYS = {"add": ("mode", "x1", "y1", "x2", "y2", "out", "expect"), "chain": ("mode", "px", "py", "op", "cols")}
    _EDWARDS_MODES = {"add": _native.KZG_EDWARDS_ADD, "chain": _native.KZG_EDWARDS_CHAIN}

    @classmethod
    def edwards_call(cls, curve, units, what: str = "commit_edwards", n_rows: Optional[int] = None) -> Tuple[tuple, List[tuple]]:
        """The kzg_edwards_curve fields (a, d as 32 big-endian bytes) and per unit the kzg_edwards_unit fields (mode, flags,
        cols, op, in[4], expect[2], out_order[2], imm[4] of 32 bytes) of a call.  curve: a mapping with a and d, the
        coefficients of A x^2 + y^2 = 1 + D x^2 y^2: canonical scalars, not 0, not equal.  A unit is a mapping.  {"mode": "add",
        "x1", "y1", "x2", "y2": slots, "out": names among x3, y3}, the output rows in the order of the names; with "expect":
        [row or None, row or None] (for x3, y3) in place of out it is a check.  {"mode": "chain", "px", "py": slots, "op": row,
        "cols": names among ax, ay}.  A slot is a row index or ("imm", value).  A scalar is an int, a decimal or 0x string, or
        32 big-endian bytes, below r.  n_rows: the number of concatenated input rows, where known: a row must lie inside.
        Raises KzgError(KZG_E_ARG) with the cause; needs no device."""
        sp = _UnitSpec(what, "edwards")
        bad = sp.bad
        ABSENT, IMM = _native.KZG_EDWARDS_ABSENT, _native.KZG_EDWARDS_IMM
        if not isinstance(curve, dict) or set(curve) != set(cls._EDWARDS_CURVE_KEYS):
            raise bad("the curve is a mapping with exactly a and d")
        a_b, d_b = sp.scalar(curve["a"], "the coefficient A"), sp.scalar(curve["d"], "the coefficient D")
        if a_b == bytes(32) or d_b == bytes(32):
            raise bad("the coefficients A and D must not be 0")
        if a_b == d_b:
            raise bad("the coefficients A and D must differ")
        recs, n_out = [], 0

        def row(v, name):
            if not _is_u(v, IMM):
                raise bad(f"{name} must be a row, an integer in [0, 2^32 - 2)")
            if n_rows is not None and v >= n_rows:
                raise bad(f"{name} reaches beyond the {n_rows} concatenated rows of the input sets")
            sp.seen.add(v)
            return v

        def slot(v, name):
            if isinstance(v, (list, tuple)):
                return sp.slot(v, name, top=IMM)
            if v is None or isinstance(v, bool) or not isinstance(v, int):
                raise bad(f'{name} must be a row index, an integer in [0, 2^32 - 2), or ("imm", value)')
            return row(v, name), bytes(32)

        for un in sp.units(units, _native.KZG_EDWARDS_MAX_UNITS):
            mode = sp.mode(un, cls._EDWARDS_KEYS, "expect belongs to add units, not to chain: a chain is never a check")
            flags, op, ins, imms, expect = 0, ABSENT, [ABSENT] * 4, [bytes(32)] * 4, [ABSENT] * 2
            if mode == "chain":
                names = _native.KZG_EDWARDS_CHAIN_NAMES
                for j, k in enumerate(("px", "py")):
                    ins[j], imms[j] = slot(un.get(k), k)
                op = row(un.get("op"), "op")
                picked = sp.names(un.get("cols"), names, lambda: f"cols must hold 1 .. 2 column names among {', '.join(names)}", "name", mode)
            else:
                names = _native.KZG_EDWARDS_ADD_NAMES
                for j, k in enumerate(("x1", "y1", "x2", "y2")):
                    ins[j], imms[j] = slot(un.get(k), k)
                if sp.out_or_expect(un):
                    ex = un["expect"]
                    if not isinstance(ex, (list, tuple)) or len(ex) != 2:
                        raise bad("expect must hold two entries (x3, y3; None: not compared)")
                    picked = [j for j, v in enumerate(ex) if v is not None]
                    if not picked:
                        raise bad("expect must name at least one row")
                    for j in picked:
                        expect[j] = row(ex[j], "an entry of expect")
                    flags |= _native.KZG_EDWARDS_CHECK
                else:
                    picked = sp.names(un["out"], names, lambda: f"out must hold 1 .. 2 names among {', '.join(names)}", "name", mode)
            if not flags:
                n_out += len(picked)
            recs.append((cls._EDWARDS_MODES[mode], flags, sum(1 << k for k in picked), op, ins, expect,
                         [ABSENT] * 2 if flags else _pad(picked, 2, ABSENT), imms))
        sp.caps(n_out)
        return (a_b, d_b), recs

    @staticmethod
    def edwards_structs(cv, recs) -> Tuple["_native.EdwardsCurve", object]:
        curve = _native.EdwardsCurve((ctypes.c_uint8 * 32)(*cv[0]), (ctypes.c_uint8 * 32)(*cv[1]))
        arr = (_native.EdwardsUnit * len(recs))()
        for u, r in zip(arr, recs):
            u.mode, u.flags, u.cols, u.op = r[0], r[1], r[2], r[3]
            u.in_[:], u.expect[:], u.out_order[:] = r[4], r[5], r[6]
            for j, b in enumerate(r[7]):
                u.imm_be32[j][:] = list(b)
        return curve, arr

    @staticmethod
    def edwards_n_out(recs) -> int:
        return sum(bin(r[2]).count("1") for r in recs if not r[1] & _native.KZG_EDWARDS_CHECK)

    def commit_edwards(self, input_sets: Sequence[object], curve: dict, units: Sequence[dict], usable: Optional[int] = None,
                       tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], dict]:
        """kzg_rows_commit_edwards over the concatenated rows of input_sets (RowSet objects or bare handles).  curve and units:
        see edwards_call.  A coordinate is one cell.  With tau = D x1 x2 y1 y2 an add unit commits the named ones of x3 = (x1
        y2 + y1 x2) / (1 + tau) and y3 = (y1 y2 - A x1 x2) / (1 - tau), zeros and `singular` on an exceptional row (tau = 1 or
        -1); with expect it commits nothing and counts the rows whose expected cells differ; a chain unit commits the named ones
        of ax, ay: the accumulator before each row's step, (0, 1) before row 0 and after an exceptional step, for the op-codes 0
        hold, 1 load, 2 add (px, py), 3 double, 4 subtract (px, py).  Returns (the new RowSet of all committed rows in unit
        order, or None when every unit is a check; {"singular", "first_singular", "mismatch", "first_mismatch", "unknown",
        "first_unknown", "segments"} per unit).  usable and tail: as for commit_derived, the tail column-major over the
        committed rows."""
        what = "commit_edwards"
        ni, hi = self._handle_array(input_sets, what)
        cv, recs = self.edwards_call(curve, units, what, self._n_rows(input_sets))
        cs, arr = self.edwards_structs(cv, recs)
        return self._commit_units(what, self._lib.kzg_rows_commit_edwards, input_sets, ni, hi, cs, arr, self.edwards_n_out(recs),
                                  usable, tail, self._CURVE_STATS, _native.KZG_EDWARDS_NONE)

    # ---- a set built from sets: columns that are plain arithmetic in resident columns, and gates checked row by row
    def commit_expr(self, input_sets: Sequence[object], exprs: Sequence[Sequence], usable: Optional[int] = None,
                    tail: Sequence[bytes] = ()) -> Tuple[Optional["RowSet"], List[int], List[Optional[int]]]:
        """kzg_rows_commit_expr over the concatenated rows of input_sets (RowSet objects or bare handles).  exprs: a list of
        (terms,) or (terms, check) entries; terms as in commit_quotient_ext: (32-byte coefficient, factors) per term, a factor a
        row index or a (row, rot) pair, at most KZG_MAX_EXPR_FACTORS per term; v[t] = sum_u c_u prod_f col[(t + rot) mod T].  An
        entry with check = True is evaluated and counted only.  Returns (the new RowSet of the committed expressions in their
        order, or None when every entry is a check; per entry the number of non-zero cells among the rows evaluated; per
        entry the smallest such row, or None).  usable = None evaluates all T rows; otherwise only rows [0, usable) and row
        usable + s of committed column c takes tail[c * (T - usable) + s] (32 bytes each, column-major; no closing row)."""
        what = "commit_expr"
        ni, hi = self._handle_array(input_sets, what)
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        exprs = list(exprs) if isinstance(exprs, (list, tuple)) else None
        if not exprs or len(exprs) > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"exprs must be a list of 1 .. {_native.KZG_MAX_BATCH_OPEN} entries")
        arr, keep, checks = (_native.Expr * len(exprs))(), [], []
        for e, ent in enumerate(exprs):
            if not isinstance(ent, (list, tuple)) or len(ent) not in (1, 2) or (len(ent) == 2 and not isinstance(ent[1], bool)):
                raise bad("an entry of exprs is (terms,) or (terms, check) with check a bool")
            try:
                tt = []
                for c, factors in ent[0]:
                    if any(isinstance(f, (tuple, list)) and len(f) != 2 for f in factors):
                        raise ValueError("a factor is a row index or a (row, rot) pair")
                    tt.append((bytes(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in factors]))
            except (TypeError, ValueError) as ex:
                raise bad(f"malformed terms: {ex!r}") from ex
            if not 1 <= len(tt) <= _native.KZG_MAX_GATE_TERMS or any(
                    len(c) != 32 or len(fs) > _native.KZG_MAX_EXPR_FACTORS for c, fs in tt):
                raise bad(f"an expression has 1 .. {_native.KZG_MAX_GATE_TERMS} terms of a 32-byte coefficient and at most "
                          f"{_native.KZG_MAX_EXPR_FACTORS} factors")
            flat = [f for _, fs in tt for f in fs]
            if any(not 0 <= j < 1 << 32 or not -(1 << 31) <= rot < 1 << 31 for j, rot in flat):
                raise bad("row indices must be non-negative integers below 2^32 and rotations must fit an int32")
            lens = (ctypes.c_uint32 * len(tt))(*[len(fs) for _, fs in tt])
            rows_arr = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
            rots_arr = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
            check = len(ent) == 2 and ent[1]
            arr[e] = _native.Expr(_native.QuotientTerms(len(tt), b"".join(c for c, _ in tt), lens, rows_arr, rots_arr),
                                  _native.KZG_EXPR_CHECK if check else 0)
            keep.append((lens, rows_arr, rots_arr))   # the arrays live as long as the structures that point at them
            checks.append(check)
        n_out = checks.count(False)
        wi, T, lay = self._column_layout(what, input_sets, n_out, "n_out", "evaluated", usable, tail)
        opts = _native.ExprOpts(*lay) if lay else None
        c, h = ctypes.create_string_buffer(48 * max(n_out, 1)), ctypes.c_uint64(0)
        nz, first = (ctypes.c_uint64 * len(exprs))(), (ctypes.c_uint64 * len(exprs))()
        self._chk(self._lib.kzg_rows_commit_expr(self._h, ni, hi, len(exprs), arr, ctypes.byref(opts) if opts is not None else None,
                                                 c if n_out else None, nz, first, ctypes.byref(h)))
        del keep
        rs = RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]) if n_out else None
        return rs, [int(v) for v in nz], [None if int(v) == _native.KZG_EXPR_NONE else int(v) for v in first]

    # ---- a set built from sets: running values along the rows, v[t + 1] = A[t] v[t] + B[t] with A and B expressions
    def commit_recurrence(self, input_sets: Sequence[object], recs: Sequence[Sequence], usable: Optional[int] = None,
                          tail: Sequence[bytes] = ()) -> Tuple["RowSet", List[bytes]]:
        """kzg_rows_commit_recurrence over the concatenated rows of input_sets (RowSet objects or bare handles).  recs: a list of
        (mul_terms, add_terms, start_be32) entries; both term lists as in commit_expr ((32-byte coefficient, factors) per term, a
        factor a row index or a (row, rot) pair), an empty mul_terms standing for A = 1 and an empty add_terms for B = 0 (not
        both); v[0] = start, v[t + 1] = A[t] v[t] + B[t].  Returns (the new RowSet of the recurrences in their order, the closing
        value of each as 32 bytes).  usable = None: rows 0 .. T - 1 hold v[0] .. v[T - 1] and the closing value is v[T];
        otherwise rows 0 .. usable hold v[0] .. v[usable], the last of them the closing value, and row usable + 1 + s of column c
        takes tail[c * (T - usable - 1) + s] (32 bytes each, column-major)."""
        what = "commit_recurrence"
        ni, hi = self._handle_array(input_sets, what)
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        recs = list(recs) if isinstance(recs, (list, tuple)) else None
        if not recs or len(recs) > _native.KZG_MAX_BATCH_OPEN:
            raise bad(f"recs must be a list of 1 .. {_native.KZG_MAX_BATCH_OPEN} entries")
        arr, keep = (_native.Recurrence * len(recs))(), []

        def side(terms):
            try:
                tt = []
                for c, factors in terms:
                    if any(isinstance(f, (tuple, list)) and len(f) != 2 for f in factors):
                        raise ValueError("a factor is a row index or a (row, rot) pair")
                    tt.append((bytes(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in factors]))
            except (TypeError, ValueError) as ex:
                raise bad(f"malformed terms: {ex!r}") from ex
            if len(tt) > _native.KZG_MAX_GATE_TERMS or any(len(c) != 32 or len(fs) > _native.KZG_MAX_EXPR_FACTORS for c, fs in tt):
                raise bad(f"an expression has at most {_native.KZG_MAX_GATE_TERMS} terms of a 32-byte coefficient and at most "
                          f"{_native.KZG_MAX_EXPR_FACTORS} factors")
            flat = [f for _, fs in tt for f in fs]
            if any(not 0 <= j < 1 << 32 or not -(1 << 31) <= rot < 1 << 31 for j, rot in flat):
                raise bad("row indices must be non-negative integers below 2^32 and rotations must fit an int32")
            if not tt:
                return _native.QuotientTerms(0, None, None, None, None)
            lens = (ctypes.c_uint32 * len(tt))(*[len(fs) for _, fs in tt])
            rows_arr = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
            rots_arr = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
            keep.append((lens, rows_arr, rots_arr))   # the arrays live as long as the structures that point at them
            return _native.QuotientTerms(len(tt), b"".join(c for c, _ in tt), lens, rows_arr, rots_arr)

        for e, ent in enumerate(recs):
            if not isinstance(ent, (list, tuple)) or len(ent) != 3 or not isinstance(ent[2], (bytes, bytearray)) or len(ent[2]) != 32:
                raise bad("an entry of recs is (mul_terms, add_terms, start) with start of 32 bytes")
            mul, add = side(ent[0]), side(ent[1])
            if mul.n_terms == 0 and add.n_terms == 0:
                raise bad("mul_terms and add_terms must not both be empty")
            arr[e] = _native.Recurrence(mul, add, bytes(ent[2]))
        wi, T, lay = self._recurrence_layout(what, input_sets, len(recs), usable, tail)
        opts = _native.RecurrenceOpts(*lay) if lay else None
        c, cl, h = ctypes.create_string_buffer(48 * len(recs)), ctypes.create_string_buffer(32 * len(recs)), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_recurrence(self._h, ni, hi, len(recs), arr, ctypes.byref(opts) if opts is not None else None,
                                                       c, cl, ctypes.byref(h)))
        del keep
        k = len(recs)
        return (RowSet(self, h.value, wi, k, T, [c.raw[48 * p:48 * p + 48] for p in range(k)]),
                [cl.raw[32 * p:32 * p + 32] for p in range(k)])

    def _recurrence_layout(self, what: str, input_sets, n_cols: int, usable, tail):
        """The usable layout WITH a closing row over n_cols columns (kzg_recurrence_opts): (worker, T, None for the plain layout or
        (usable, the column-major tail's bytes or None)); worker and T are None for bare handles of sets this engine did not
        commit, which only the plain layout accepts."""
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        tail = [bytes(x) for x in (tail or [])]
        src = next((x for x in input_sets if getattr(x, "T", None) is not None), None)
        wi, T = (src.i, src.T) if src is not None else next(
            (self._set_len[int(x)] for x in input_sets if not hasattr(x, "handle") and int(x) in self._set_len), (None, None))
        if usable is None:
            if tail:
                raise bad("a tail needs usable (None: the plain layout)")
            return wi, T, None
        if not isinstance(usable, int) or not 1 <= usable < 1 << 64:   # (the C call reads 0 as "plain layout": here None)
            raise bad("usable must be in [1, T - 1] (None: the plain layout)")
        if any(len(x) != 32 for x in tail):
            raise bad("the tail scalars must be of 32 bytes each")
        if T is None:
            raise bad("the row length of the sets is unknown to this engine (they were not committed through it)")
        if usable < T and T - usable <= _native.KZG_MAX_BLIND_ROWS and len(tail) != n_cols * (T - usable - 1):
            raise bad(f"the tail must hold exactly n_recs * (T - usable - 1) = {n_cols * (T - usable - 1)} scalars, not {len(tail)}")
        return wi, T, (usable, b"".join(tail) if tail else None)

    # ---- a set built from sets: columns read out of a resident table, by key or by row index
    def commit_fetch(self, input_sets: Sequence[object], table_sets: Sequence[object], n_reads: int, n_keys: int,
                     with_index: bool = False, usable: Optional[int] = None,
                     tail: Sequence[bytes] = ()) -> Tuple["RowSet", List[int], List[Optional[int]]]:
        """kzg_rows_commit_fetch.  The concatenated rows of table_sets are the table's columns: the first n_keys the key, the
        others the payload.  The concatenated rows of input_sets are n_reads reads of n_keys rows each (read-major); with n_keys
        = 0 a read is ONE row of row indices and every table column is payload.  Each cell takes the payload of the smallest
        table row whose key equals the cell's key (with_index: that row number first), or zeros where there is none.  Returns
        (the new RowSet of n_reads * (payload columns + with_index) rows in read order, per read the number of cells without a
        table row, per read the smallest such cell or None).  usable = None reads all T rows; otherwise only cells and table
        rows [0, usable) take part and row usable + s of output column c takes tail[c * (T - usable) + s] (32 bytes each,
        column-major; there is no closing row)."""
        what = "commit_fetch"
        ni, hi = self._handle_array(input_sets, f"{what} (inputs)")
        nt, ht = self._handle_array(table_sets, f"{what} (table)")
        bad = lambda why: KzgError(_native.KZG_E_ARG, f"{what}: {why}")   # noqa: E731
        cap = _native.KZG_MAX_BATCH_OPEN
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (n_reads, n_keys)) or not isinstance(with_index, bool):
            raise bad("n_reads and n_keys must be integers and with_index a bool")
        if not 1 <= n_reads <= cap or not 0 <= n_keys <= cap or n_reads * max(n_keys, 1) > cap:
            raise bad(f"n_reads >= 1, n_keys >= 0, n_reads * max(n_keys, 1) <= {cap}")
        if with_index and n_keys == 0:
            raise bad("with_index needs n_keys >= 1 (by row index the address column is the index)")
        widths = [x.k if hasattr(x, "handle") else self._set_rows.get(int(x)) for x in table_sets]
        if any(k is None for k in widths):   # (n_out sizes the tail and the RowSet that is returned)
            raise bad("the row count of the table sets is unknown to this engine (they were not committed through it)")
        w_tab = sum(widths)
        if n_keys > w_tab:
            raise bad(f"n_keys = {n_keys} exceeds the {w_tab} table rows")
        n_out = n_reads * (w_tab - n_keys + int(with_index))
        if not 1 <= n_out <= cap:
            raise bad(f"n_reads * (payload rows + with_index) = {n_out} output rows must be in [1, {cap}]")
        wi, T, lay = self._column_layout(what, list(input_sets) + list(table_sets), n_out, "n_out", "read", usable, tail)
        opts = _native.DeriveOpts(*lay) if lay else None
        c, h = ctypes.create_string_buffer(48 * cap), ctypes.c_uint64(0)
        miss, first = (ctypes.c_uint64 * n_reads)(), (ctypes.c_uint64 * n_reads)()
        self._chk(self._lib.kzg_rows_commit_fetch(self._h, ni, hi, nt, ht, n_reads, n_keys,
                                                  _native.KZG_FETCH_INDEX if with_index else 0,
                                                  ctypes.byref(opts) if opts is not None else None, c, miss, first, ctypes.byref(h)))
        return (RowSet(self, h.value, wi, n_out, T, [c.raw[48 * p:48 * p + 48] for p in range(n_out)]), [int(v) for v in miss],
                [None if int(v) == _native.KZG_FETCH_NONE else int(v) for v in first])

    # ---- a third set built from sets: the PLONK quotient (round 3), computed and committed on the device
    def commit_quotient(self, sets: Sequence[object], terms: Sequence[Tuple[bytes, Sequence[int]]], perm: Optional[dict] = None,
                        ext_log: int = 2, n_pieces: int = 3) -> "RowSet":
        """The pieces of t = (Gate + alpha P1 + alpha^2 P2) / (X^T - 1) of kzg_rows_commit_quotient over the concatenated rows
        of `sets` (RowSet objects or bare handles), as a new RowSet of n_pieces rows.  terms: (32-byte coefficient, row
        indices) per gate term; perm: None, or a dict with "wires", "sigmas" (k row indices each), "z" (a row index),
        "shifts" (k x 32 bytes), "beta", "gamma", "alpha" (32 bytes each); k = 0 (no wire) switches the part off like None.
        alpha must be drawn after z's commitment is
        fixed, beta and gamma after the wires.  KZG_E_ARG when t does not fit n_pieces rows (the constraints do not hold on
        the domain, or n_pieces is too small)."""
        n, hs = self._handle_array(sets, "commit_quotient")
        bad = lambda why: KzgError(_native.KZG_E_ARG, "commit_quotient: " + why)   # noqa: E731
        if ext_log not in (1, 2, 3) or not 1 <= n_pieces <= 1 << ext_log:
            raise bad("ext_log must be 1, 2 or 3 and n_pieces in [1, 2^ext_log]")
        E = 1 << ext_log
        terms = [(bytes(c), [int(j) for j in rows]) for c, rows in terms]
        if len(terms) > _native.KZG_MAX_GATE_TERMS or any(len(c) != 32 or len(rows) > E + 1 for c, rows in terms):
            raise bad(f"at most {_native.KZG_MAX_GATE_TERMS} terms of a 32-byte coefficient and at most 2^ext_log + 1 rows")
        gate_rows = [j for _, rows in terms for j in rows]
        if any(not 0 <= j < 1 << 32 for j in gate_rows):
            raise bad("row indices must be non-negative integers below 2^32")
        lens = (ctypes.c_uint32 * max(len(terms), 1))(*[len(rows) for _, rows in terms])
        gate = _native.QuotientGate(len(terms), b"".join(c for c, _ in terms), lens, None)
        pm = None
        if perm is not None:
            try:
                wires, sigmas = [int(j) for j in perm["wires"]], [int(j) for j in perm["sigmas"]]
                k = len(wires)
                if k:   # (k == 0 switches the part off, as perm->k == 0 does: nothing else of perm is read)
                    shifts, z = list(perm["shifts"]), int(perm["z"])
                    scal = shifts + [perm["beta"], perm["gamma"], perm["alpha"]]
            except (KeyError, TypeError, ValueError) as e:
                raise bad(f"malformed permutation part: {e!r}") from e
            if k:
                if k > E or len(sigmas) != k or len(shifts) != k or any(len(x) != 32 for x in scal):
                    raise bad("the permutation part takes at most 2^ext_log wires, as many sigmas and shifts, and 32-byte scalars")
                if any(not 0 <= j < 1 << 32 for j in wires + sigmas + [z]):
                    raise bad("row indices must be non-negative integers below 2^32")
                pm = _native.QuotientPerm(k, z, (ctypes.c_uint32 * k)(*wires), (ctypes.c_uint32 * k)(*sigmas),
                                          b"".join(shifts), perm["beta"], perm["gamma"], perm["alpha"])
            elif sigmas:
                raise bad("the permutation part names sigma rows but no wire")
        if not terms and pm is None:
            raise bad("no gate term and no permutation part")
        rows_arr = (ctypes.c_uint32 * max(len(gate_rows), 1))(*gate_rows)
        gate.term_rows = ctypes.cast(rows_arr, ctypes.POINTER(ctypes.c_uint32))
        c, h = ctypes.create_string_buffer(48 * n_pieces), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_quotient(self._h, n, hs, ctypes.byref(gate), ctypes.byref(pm) if pm is not None else None,
                                                     ext_log, n_pieces, c, ctypes.byref(h)))
        src = next((x for x in sets if hasattr(x, "T")), None)
        return RowSet(self, h.value, getattr(src, "i", None), n_pieces, getattr(src, "T", None),
                      [c.raw[48 * p:48 * p + 48] for p in range(n_pieces)])

    # ---- the same with rotated gate factors and the logUp relation (what makes commit_lookup_sum's S an argument)
    def commit_quotient_ext(self, sets: Sequence[object], terms: Sequence[Tuple[bytes, Sequence[object]]],
                            perm: Optional[dict] = None, lookup: Optional[dict] = None, ext_log: int = 2,
                            n_pieces: int = 3) -> "RowSet":
        """The pieces of t = (Gate + alpha P1 + alpha^2 P2 + alpha^3 LK1 + alpha^4 LK2) / (X^T - 1) of
        kzg_rows_commit_quotient_ext.  sets, perm, ext_log and n_pieces as in commit_quotient.  terms: (32-byte coefficient,
        factors) per gate term, a factor being a row index or a (row, rot) pair: the row at w^rot X, i.e. at t + rot on the
        domain (any int32 rot, reduced mod T).  lookup: None, or a dict with "inputs" (n_lookups * width row indices,
        lookup-major), "table" (width row indices), "mult", "sum" (row indices of m and S), "width", and "theta", "beta",
        "alpha" (32 bytes each; theta and beta those S was built with, alpha the one of perm).  n_lookups <= 2^ext_log - 1.
        alpha must be drawn after the commitments of S and z are fixed."""
        return self._commit_quotient_ext("commit_quotient_ext", sets, terms, perm, lookup, None, ext_log, n_pieces)

    def commit_quotient_zk(self, sets: Sequence[object], terms: Sequence[Tuple[bytes, Sequence[object]]],
                           perm: Optional[dict] = None, lookup: Optional[dict] = None, active_row: Optional[int] = None,
                           ext_log: int = 2, n_pieces: int = 3) -> "RowSet":
        """commit_quotient_ext with the caller's active column (kzg_rows_commit_quotient_zk): row active_row of the
        concatenation, 1 on the usable rows and 0 elsewhere, multiplies P1 and LK1, so that neither binds the blinding rows.
        The permutation part then takes at most 2^ext_log - 1 wires and the lookup part at most 2^ext_log - 2 lookups.
        active_row = None is commit_quotient_ext."""
        return self._commit_quotient_ext("commit_quotient_zk", sets, terms, perm, lookup, active_row, ext_log, n_pieces)

    def _quotient_selectors(self, what, selectors, lk):
        """The ctypes form of a selector list (one entry per lookup: None or a row index of the concatenation), or None."""
        if selectors is None:
            return None
        bad = lambda why: KzgError(_native.KZG_E_ARG, what + ": " + why)   # noqa: E731
        if lk is None:
            raise bad("selectors need a lookup part")
        idx = [_native.KZG_NO_SELECTOR if j is None else j for j in selectors]
        if len(idx) != lk.n_lookups or any(not isinstance(j, int) or not 0 <= j <= _native.KZG_NO_SELECTOR for j in idx):
            raise bad("selectors must hold n_lookups entries, each None or a row index")
        arr = (ctypes.c_uint32 * len(idx))(*idx)
        sel = _native.QuotientSelectors(arr)
        sel._keep = arr
        return sel

    def commit_quotient_sel(self, sets: Sequence[object], terms: Sequence[Tuple[bytes, Sequence[object]]],
                            perm: Optional[dict] = None, lookup: Optional[dict] = None,
                            selectors: Optional[Sequence[Optional[int]]] = None, active_row: Optional[int] = None,
                            ext_log: int = 2, n_pieces: int = 3) -> "RowSet":
        """commit_quotient_zk with per-row lookup selectors (kzg_rows_commit_quotient_sel): selectors[l] is the row of the
        concatenation that holds q_l, the numerator of lookup l's fraction in LK1, or None (the constant 1).  selectors = None,
        or all None, is commit_quotient_zk."""
        what = "commit_quotient_sel"
        n, hs, gate, pm, lk, act = self._quotient_args(what, sets, terms, perm, lookup, active_row, ext_log, n_pieces)
        sel = self._quotient_selectors(what, selectors, lk)
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        c, h = ctypes.create_string_buffer(48 * n_pieces), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_commit_quotient_sel(self._h, n, hs, ctypes.byref(gate), ref(pm), ref(lk), ref(sel), ref(act),
                                                         ext_log, n_pieces, c, ctypes.byref(h)))
        src = next((x for x in sets if hasattr(x, "T")), None)
        return RowSet(self, h.value, getattr(src, "i", None), n_pieces, getattr(src, "T", None),
                      [c.raw[48 * p:48 * p + 48] for p in range(n_pieces)])

    def quotient_part_sel(self, sets, terms, perm=None, lookup=None, selectors=None, active_row=None, link=None, ext_log: int = 2,
                          scale_be32: Optional[bytes] = None, acc: Optional["QuotientAcc"] = None) -> "QuotientAcc":
        """quotient_part with per-row lookup selectors (kzg_rows_quotient_part_sel); selectors as in commit_quotient_sel."""
        return self.quotient_part(sets, terms, perm, lookup, active_row, link, ext_log, scale_be32, acc, _selectors=selectors,
                                  _what="quotient_part_sel")

    def _commit_quotient_ext(self, what, sets, terms, perm, lookup, active_row, ext_log, n_pieces) -> "RowSet":
        n, hs, gate, pm, lk, act = self._quotient_args(what, sets, terms, perm, lookup, active_row, ext_log, n_pieces)
        c, h = ctypes.create_string_buffer(48 * n_pieces), ctypes.c_uint64(0)
        pm_ref = ctypes.byref(pm) if pm is not None else None
        lk_ref = ctypes.byref(lk) if lk is not None else None
        if act is None:
            self._chk(self._lib.kzg_rows_commit_quotient_ext(self._h, n, hs, ctypes.byref(gate), pm_ref, lk_ref, ext_log,
                                                             n_pieces, c, ctypes.byref(h)))
        else:
            self._chk(self._lib.kzg_rows_commit_quotient_zk(self._h, n, hs, ctypes.byref(gate), pm_ref, lk_ref, ctypes.byref(act),
                                                            ext_log, n_pieces, c, ctypes.byref(h)))
        src = next((x for x in sets if hasattr(x, "T")), None)
        return RowSet(self, h.value, getattr(src, "i", None), n_pieces, getattr(src, "T", None),
                      [c.raw[48 * p:48 * p + 48] for p in range(n_pieces)])

    def _quotient_args(self, what, sets, terms, perm, lookup, active_row, ext_log, n_pieces):
        """The checks and the ctypes forms shared by commit_quotient_ext / _zk and quotient_part (n_pieces None: a part has
        none): (n, handles, QuotientTerms, QuotientPerm or None, QuotientLookup or None, QuotientActive or None)."""
        n, hs = self._handle_array(sets, what)
        bad = lambda why: KzgError(_native.KZG_E_ARG, what + ": " + why)   # noqa: E731
        if active_row is not None and (not isinstance(active_row, int) or not 0 <= active_row < 1 << 32):
            raise bad("active_row must be a non-negative integer below 2^32")
        if ext_log not in (1, 2, 3) or (n_pieces is not None and not 1 <= n_pieces <= 1 << ext_log):
            raise bad("ext_log must be 1, 2 or 3 and n_pieces in [1, 2^ext_log]")
        E = 1 << ext_log
        try:
            tt = []
            for c, factors in terms:
                fs = [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in factors]
                if any(isinstance(f, (tuple, list)) and len(f) != 2 for f in factors):
                    raise ValueError("a factor is a row index or a (row, rot) pair")
                tt.append((bytes(c), fs))
        except (TypeError, ValueError) as e:
            raise bad(f"malformed terms: {e!r}") from e
        if len(tt) > _native.KZG_MAX_GATE_TERMS or any(len(c) != 32 or len(fs) > E + 1 for c, fs in tt):
            raise bad(f"at most {_native.KZG_MAX_GATE_TERMS} terms of a 32-byte coefficient and at most 2^ext_log + 1 factors")
        flat = [f for _, fs in tt for f in fs]
        if any(not 0 <= j < 1 << 32 or not -(1 << 31) <= rot < 1 << 31 for j, rot in flat):
            raise bad("row indices must be non-negative integers below 2^32 and rotations must fit an int32")
        pm = None
        if perm is not None:
            try:
                wires, sigmas = [int(j) for j in perm["wires"]], [int(j) for j in perm["sigmas"]]
                k = len(wires)
                if k:
                    shifts, z = list(perm["shifts"]), int(perm["z"])
                    scal = shifts + [perm["beta"], perm["gamma"], perm["alpha"]]
            except (KeyError, TypeError, ValueError) as e:
                raise bad(f"malformed permutation part: {e!r}") from e
            if k:
                if k > E or len(sigmas) != k or len(shifts) != k or any(len(x) != 32 for x in scal):
                    raise bad("the permutation part takes at most 2^ext_log wires, as many sigmas and shifts, and 32-byte scalars")
                if any(not 0 <= j < 1 << 32 for j in wires + sigmas + [z]):
                    raise bad("row indices must be non-negative integers below 2^32")
                pm = _native.QuotientPerm(k, z, (ctypes.c_uint32 * k)(*wires), (ctypes.c_uint32 * k)(*sigmas),
                                          b"".join(shifts), perm["beta"], perm["gamma"], perm["alpha"])
            elif sigmas:
                raise bad("the permutation part names sigma rows but no wire")
        lk = None
        if lookup is not None:
            try:
                ins, tab = [int(j) for j in lookup["inputs"]], [int(j) for j in lookup["table"]]
                w, mrow, srow = int(lookup["width"]), int(lookup["mult"]), int(lookup["sum"])
                lscal = [bytes(lookup[name]) for name in ("theta", "beta", "alpha")]
            except (KeyError, TypeError, ValueError) as e:
                raise bad(f"malformed lookup part: {e!r}") from e
            if w < 1 or len(tab) != w or not ins or len(ins) % w or len(ins) > _native.KZG_MAX_BATCH_OPEN:
                raise bad(f"the lookup part takes width >= 1 table rows and n_lookups * width <= {_native.KZG_MAX_BATCH_OPEN} "
                          "input rows, n_lookups >= 1")
            if len(ins) // w > E - 1:
                raise bad("the lookup part has n_lookups + 2 factors: n_lookups must not exceed 2^ext_log - 1")
            if any(len(x) != 32 for x in lscal) or any(not 0 <= j < 1 << 32 for j in ins + tab + [mrow, srow]):
                raise bad("the lookup part takes 32-byte scalars and non-negative row indices below 2^32")
            if pm is not None and lscal[2] != bytes(perm["alpha"]):
                raise bad("the permutation part and the lookup part must name one alpha")
            lk = _native.QuotientLookup(len(ins) // w, w, (ctypes.c_uint32 * len(ins))(*ins), (ctypes.c_uint32 * w)(*tab), mrow,
                                        srow, *lscal)
        if not tt and pm is None and lk is None:
            raise bad("no gate term, no permutation part and no lookup part")
        lens = (ctypes.c_uint32 * max(len(tt), 1))(*[len(fs) for _, fs in tt])
        rows_arr = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
        rots_arr = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
        gate = _native.QuotientTerms(len(tt), b"".join(c for c, _ in tt), lens, rows_arr, rots_arr)
        gate._keep = (lens, rows_arr, rots_arr)   # the arrays live as long as the structure that points at them
        return n, hs, gate, pm, lk, (None if active_row is None else _native.QuotientActive(active_row))

    # ---- the quotient in parts: circuits that fit no single call (more than 16 rows, more permuted columns than 2^ext_log - 1,
    # several permutation or lookup arguments) sum their numerator on the device over several calls
    def quotient_part(self, sets: Sequence[object], terms: Sequence[Tuple[bytes, Sequence[object]]], perm: Optional[dict] = None,
                      lookup: Optional[dict] = None, active_row: Optional[int] = None, link: Optional[Tuple[int, int]] = None,
                      ext_log: int = 2, scale_be32: Optional[bytes] = None, acc: Optional["QuotientAcc"] = None,
                      _selectors=None, _what: str = "quotient_part") -> "QuotientAcc":
        """One part of a quotient (kzg_rows_quotient_part): this part's numerator over the concatenated rows of `sets`, with
        terms, perm, lookup and active_row as in commit_quotient_zk and its own row numbering, divided by Z_H on the coset,
        multiplied by scale_be32 (32 bytes, None: 1) and added into `acc` (None: a new accumulator).  link: None, or (prev_row,
        rot): P2 becomes (z(X) - f_prev(w^rot X)) L_0(X), the chain relation of a chunked permutation (needs perm).  Returns
        the accumulator (a QuotientAcc; the one passed in, or the new one); quotient_finish turns it into the pieces.  Each part
        re-extends the rows it names."""
        n, hs, gate, pm, lk, act = self._quotient_args(_what, sets, terms, perm, lookup, active_row, ext_log, None)
        sel = self._quotient_selectors(_what, _selectors, lk)
        bad = lambda why: KzgError(_native.KZG_E_ARG, _what + ": " + why)   # noqa: E731
        ln = None
        if link is not None:
            try:
                prev_row, rot = int(link[0]), int(link[1])
                if len(link) != 2:
                    raise ValueError("a link is a (prev_row, rot) pair")
            except (TypeError, ValueError, IndexError) as e:
                raise bad(f"malformed link: {e!r}") from e
            if not 0 <= prev_row < 1 << 32 or not -(1 << 31) <= rot < 1 << 31:
                raise bad("the link's row must be a non-negative integer below 2^32 and its rotation must fit an int32")
            if pm is None:
                raise bad("a link needs a permutation part")
            ln = _native.QuotientLink(prev_row, rot)
        if scale_be32 is not None and len(scale_be32) != 32:
            raise bad("scale must be 32 bytes or None")
        if acc is not None and not isinstance(acc, QuotientAcc):
            raise bad("acc must be a QuotientAcc returned by quotient_part, or None")
        h = ctypes.c_uint64(0 if acc is None else acc.handle)
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        if _selectors is None:
            self._chk(self._lib.kzg_rows_quotient_part(self._h, n, hs, ctypes.byref(gate), ref(pm), ref(ln), ref(lk), ref(act),
                                                       ext_log, scale_be32, ctypes.byref(h)))
        else:
            self._chk(self._lib.kzg_rows_quotient_part_sel(self._h, n, hs, ctypes.byref(gate), ref(pm), ref(ln), ref(lk), ref(sel),
                                                           ref(act), ext_log, scale_be32, ctypes.byref(h)))
        if acc is not None:
            return acc
        src = next((x for x in sets if hasattr(x, "T")), None)
        i, T = (src.i, src.T) if src is not None else next(
            (self._set_len[int(x)] for x in sets if not hasattr(x, "handle") and int(x) in self._set_len), (None, None))
        return QuotientAcc(self, h.value, i, T, ext_log)

    def quotient_finish(self, acc: "QuotientAcc", n_pieces: int = 3) -> "RowSet":
        """The pieces of the accumulated quotient (kzg_rows_quotient_finish) as a new RowSet of n_pieces rows; the accumulator
        is consumed.  KzgError(KZG_E_ARG) when t does not fit n_pieces rows (the constraints do not hold, or n_pieces is too
        small): no set is created then and the accumulator stays live, for the caller to release."""
        if not isinstance(acc, QuotientAcc):
            raise KzgError(_native.KZG_E_ARG, "quotient_finish: acc must be a QuotientAcc returned by quotient_part")
        if not isinstance(n_pieces, int) or not 1 <= n_pieces <= 8:
            raise KzgError(_native.KZG_E_ARG, "quotient_finish: n_pieces must be in [1, 2^ext_log]")
        c, h = ctypes.create_string_buffer(48 * n_pieces), ctypes.c_uint64(0)
        self._chk(self._lib.kzg_rows_quotient_finish(self._h, acc.handle, n_pieces, c, ctypes.byref(h)))
        acc.released = True   # consumed: its handle is dead
        return RowSet(self, h.value, acc.i, n_pieces, acc.T, [c.raw[48 * p:48 * p + 48] for p in range(n_pieces)])

    def commit_grand_product_chain(self, wire_sets: Sequence[object], sigma_sets: Sequence[object], shifts_be32: Sequence[bytes],
                                   beta_be32: bytes, gamma_be32: bytes, usable: int, tail_be32: Sequence[bytes],
                                   start_be32: bytes) -> Tuple["RowSet", bytes]:
        """commit_grand_product_zk whose z starts at start_be32 instead of 1 (kzg_rows_commit_grand_product_chain): the chunk of
        a chained permutation.  z(w^usable) = start * prod N / prod D is the closing value, the next chunk's start; the tail is
        untouched by start.  start must be canonical and not 0."""
        return self._grand_product("commit_grand_product_chain", wire_sets, sigma_sets, shifts_be32, beta_be32, gamma_be32,
                                   (usable, tail_be32), start_be32)

    def _handle_array(self, sets, what):
        handles = [int(getattr(x, "handle", x)) for x in sets]
        n = len(handles)
        if n == 0 or n > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"{what}: {n} sets, expected 1 .. {_native.KZG_MAX_BATCH_OPEN}")
        return n, (ctypes.c_uint64 * n)(*handles)

    def verify_open_lincomb(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                            coeffs: Sequence[Sequence[bytes]], values32: Sequence[bytes], proofs48: Sequence[bytes]) -> bool:
        """Pairing check of one caller-weighted opening (open_rows_lincomb) against resident slice i."""
        if self.verifier is None:
            raise NotImplementedError("no verifier key: call set_verifier_key() after load_srs()")
        return self.verifier.verify_open_lincomb(i, commitments48, points32, coeffs, values32, proofs48)

    def release_rows(self, handle: int) -> None:
        """Frees a committed set (kzg_rows_release); KzgError(KZG_E_ARG) for an unknown or already released handle."""
        self._chk(self._lib.kzg_rows_release(self._h, int(handle)))
        self._set_len.pop(int(handle), None)
        getattr(self, "_set_rows", {}).pop(int(handle), None)

    def rows_stats(self) -> Tuple[int, int]:
        """(live committed sets, device bytes their rows hold)."""
        arr = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.kzg_rows_stats(self._h, arr))
        return arr[0], arr[1]

    # ---- the same three calls fed from the synapse's List[str] (reference neurons/miner.py:38-61): the text is decoded
    # by csrc/wire_py.c straight into the library's pinned staging buffer (no bytes object, no pageable bounce)
    class _Staged:
        """One pinned staging buffer of the library's pool holding the decoded polynomial; released on exit.  Concurrent
        requests (the axon's worker threads) each hold their own buffer, so their decodes and GPU calls overlap."""

        def __init__(self, eng: "HipEngine", poly: Sequence[str], tagged: bool = False):
            from . import codec

            if codec._wire is None:
                raise RuntimeError("zkp_subnet_amd._wire is not built: run `python -m zkp_subnet_amd.build`")
            self.eng, self.n = eng, len(poly)
            ptr, tok = ctypes.c_void_p(), ctypes.c_int(-1)
            eng._chk(eng._lib.kzg_staging_acquire(eng._h, 32 * max(self.n, 1), ctypes.byref(ptr), ctypes.byref(tok)))
            self.token = tok.value
            cap = 32 * max(self.n, 1)
            try:
                tile = max(HipEngine.STREAM_TILE, self.n >> 2)
                if not tagged and self.n >= HipEngine.STREAM_MIN and self.n % tile == 0:
                    # long rows of the fused call: decode in (at most four) tiles and start each tile's upload at once
                    # (kzg_staging_flush): the copy engine moves tile k while the pool decodes tile k + 1, and the compute
                    # call finds the row on the device.  Short rows: the per-tile calls would cost what the overlap gives.
                    # Tagged calls (the two-call route) decode in one shot: the tag -- hit or miss -- is only known at
                    # the end, a hit's upload is off the critical path anyway, and tiles cost the decode ~0.1 ms each
                    # (measured: profiles/r04_ab_streamed_upload.log).
                    got, self.tag = 0, None
                    for first in range(0, self.n, tile):
                        got += codec._wire.decode_fr_list_into(poly, ptr.value, cap, 0, first, tile)
                        eng._chk(eng._lib.kzg_staging_flush(eng._h, self.token, 32 * first, 32 * tile))
                elif tagged:   # one pass: base64 -> bytes in the pinned buffer + the 128-bit content tag of those bytes
                    got, self.tag = codec._wire.decode_fr_list_into_tagged(poly, ptr.value, cap)
                else:        # fused / one-shot calls have no use for the tag (it costs ~0.7 ns per element and thread)
                    got, self.tag = codec._wire.decode_fr_list_into(poly, ptr.value, cap), None
            except ValueError as e:
                eng._lib.kzg_staging_release(eng._h, self.token)
                raise codec.CodecError(str(e)) from e
            except BaseException:
                eng._lib.kzg_staging_release(eng._h, self.token)
                raise
            assert got == self.n
            self.row = ctypes.cast(ptr, ctypes.c_char_p)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.eng._lib.kzg_staging_release(self.eng._h, self.token)
            return False

    def commit_list(self, i: int, poly: Sequence[str], evaluation_form: bool = True) -> bytes:
        out = ctypes.create_string_buffer(48)
        # tagged: the coefficient vector stays on the device for the worker_open that follows with the same row
        # (the unchanged reference miner's two-call route, neurons/miner.py:56-61)
        with HipEngine._Staged(self, poly, tagged=True) as st:
            self._chk(self._lib.kzg_commit_cached(self._h, i, st.row, st.n, int(evaluation_form), st.tag, out))
        return out.raw

    def open_list(self, i: int, poly: Sequence[str], alpha_be32: bytes, evaluation_form: bool = True) -> Tuple[bytes, bytes]:
        ev, pf = ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        with HipEngine._Staged(self, poly, tagged=True) as st:
            self._chk(self._lib.kzg_open_cached(self._h, i, st.row, st.n, int(evaluation_form), st.tag, alpha_be32, ev, pf))
        return ev.raw, pf.raw

    def commit_open_list(self, i: int, poly: Sequence[str], alpha_be32: bytes,
                         evaluation_form: bool = True) -> Tuple[bytes, bytes, bytes]:
        c, ev, pf = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        with HipEngine._Staged(self, poly) as st:
            self._chk(self._lib.kzg_commit_open(self._h, i, st.row, st.n, int(evaluation_form), alpha_be32, c, ev, pf))
        return c.raw, ev.raw, pf.raw

    def commit_open_batch_list(self, i: int, polys: Sequence[Sequence[str]], alpha_be32: bytes, gamma_be32: bytes,
                               evaluation_form: bool = True) -> Tuple[List[bytes], List[bytes], bytes]:
        """commit_open_batch fed from the synapse's text rows: the k lists are decoded by csrc/wire_py.c straight into ONE
        pinned staging buffer, row j at offset 32 T j (no bytes object in between)."""
        from . import codec

        if codec._wire is None:
            raise RuntimeError("zkp_subnet_amd._wire is not built: run `python -m zkp_subnet_amd.build`")
        k = len(polys)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"commit_open_batch: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        T = len(polys[0])
        if any(len(p) != T for p in polys):
            raise codec.CodecError("commit_open_batch: rows of unequal length")
        cap = 32 * max(k * T, 1)
        ptr, tok = ctypes.c_void_p(), ctypes.c_int(-1)
        self._chk(self._lib.kzg_staging_acquire(self._h, cap, ctypes.byref(ptr), ctypes.byref(tok)))
        try:
            for j, p in enumerate(polys):
                try:
                    got = codec._wire.decode_fr_list_into(p, ptr.value + 32 * T * j, cap - 32 * T * j)
                except ValueError as e:
                    raise codec.CodecError(str(e)) from e
                assert got == T
            return self._commit_open_batch(i, k, ctypes.cast(ptr, ctypes.c_char_p), T, alpha_be32, gamma_be32,
                                           evaluation_form)
        finally:
            self._lib.kzg_staging_release(self._h, tok.value)

    def commit_open_multi_list(self, i: int, polys: Sequence[Sequence[str]], points_be32: Sequence[bytes],
                               opened: Sequence[Sequence[int]], gammas_be32: Sequence[bytes], evaluation_form: bool = True
                               ) -> Tuple[List[bytes], List[List[bytes]], List[bytes]]:
        """commit_open_multi fed from the synapse's text rows: decoded by csrc/wire_py.c straight into ONE pinned staging
        buffer, row j at offset 32 T j (as commit_open_batch_list)."""
        from . import codec

        if codec._wire is None:
            raise RuntimeError("zkp_subnet_amd._wire is not built: run `python -m zkp_subnet_amd.build`")
        k = len(polys)
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"commit_open_multi: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        T = len(polys[0])
        if any(len(p) != T for p in polys):
            raise codec.CodecError("commit_open_multi: rows of unequal length")
        cap = 32 * max(k * T, 1)
        ptr, tok = ctypes.c_void_p(), ctypes.c_int(-1)
        self._chk(self._lib.kzg_staging_acquire(self._h, cap, ctypes.byref(ptr), ctypes.byref(tok)))
        try:
            for j, p in enumerate(polys):
                try:
                    got = codec._wire.decode_fr_list_into(p, ptr.value + 32 * T * j, cap - 32 * T * j)
                except ValueError as e:
                    raise codec.CodecError(str(e)) from e
                assert got == T
            return self._commit_open_multi(i, k, ctypes.cast(ptr, ctypes.c_char_p), T, points_be32, opened, gammas_be32,
                                           evaluation_form)
        finally:
            self._lib.kzg_staging_release(self._h, tok.value)

    def row_cache_stats(self) -> Tuple[int, int]:
        """(hits, misses) of the coefficient cache behind commit_list / open_list."""
        arr = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.kzg_row_cache_stats(self._h, arr))
        return int(arr[0]), int(arr[1])

    def msm(self, scalars_be32: bytes, srs_offset: int = 0) -> bytes:
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_msm(self._h, scalars_be32, len(scalars_be32) // 32, srs_offset, out))
        return out.raw

    def msm_partial(self, scalars_be32: bytes, srs_offset: int = 0) -> bytes:
        out = ctypes.create_string_buffer(192)
        self._chk(self._lib.kzg_msm_partial(self._h, scalars_be32, len(scalars_be32) // 32, srs_offset, out))
        return out.raw

    def g1_sum(self, partials_xyzz192: bytes) -> bytes:
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_g1_sum(self._h, partials_xyzz192, len(partials_xyzz192) // 192, out))
        return out.raw

    def g1_sum_compressed(self, points_c48: bytes) -> bytes:
        """Sum of 48-byte compressed G1 points (Pianist master aggregation sum_i commit_i) -> 48 bytes."""
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_g1_sum_compressed(self._h, points_c48, len(points_c48) // 48, out))
        return out.raw

    def set_host_finish(self, enable: bool) -> None:
        """True (default): the result point's affine conversion + compression run on the host; False: on the GPU."""
        self._chk(self._lib.kzg_set_host_finish(self._h, int(enable)))

    def ntt(self, vals_be32: bytes, inverse: bool) -> bytes:
        buf = ctypes.create_string_buffer(vals_be32, len(vals_be32))
        self._chk(self._lib.kzg_ntt(self._h, buf, len(vals_be32) // 32, int(inverse)))
        return buf.raw

    def eval(self, coeffs_be32: bytes, x_be32: bytes) -> bytes:
        out = ctypes.create_string_buffer(32)
        self._chk(self._lib.kzg_eval(self._h, coeffs_be32, len(coeffs_be32) // 32, x_be32, out))
        return out.raw

    def ntt_eval(self, vals_be32: bytes, inverse: bool, x_be32: bytes) -> bytes:
        """y = (NTT / inverse NTT of vals)(x) in one call: the coefficients never leave the device."""
        out = ctypes.create_string_buffer(32)
        self._chk(self._lib.kzg_ntt_eval(self._h, vals_be32, len(vals_be32) // 32, int(inverse), x_be32, out))
        return out.raw

    def ntt_eval_list(self, poly: Sequence[str], inverse: bool, x_be32: bytes) -> bytes:
        """The same, fed from the wire text (decoded straight into a pinned staging buffer)."""
        out = ctypes.create_string_buffer(32)
        with HipEngine._Staged(self, poly) as st:
            self._chk(self._lib.kzg_ntt_eval(self._h, st.row, st.n, int(inverse), x_be32, out))
        return out.raw

    # ------------------------------------------------------------------ device-resident inputs
    def upload_fr(self, slot: int, be32: bytes, to_mont: bool) -> None:
        self._chk(self._lib.kzg_upload_fr(self._h, slot, be32, len(be32) // 32, int(to_mont)))

    def msm_resident(self, slot: int, n: int, srs_offset: int = 0) -> bytes:
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_msm_resident(self._h, slot, n, srs_offset, out))
        return out.raw

    def msm_partial_resident(self, slot: int, n: int, srs_offset: int = 0) -> bytes:
        out = ctypes.create_string_buffer(192)
        self._chk(self._lib.kzg_msm_partial_resident(self._h, slot, n, srs_offset, out))
        return out.raw

    def msm_submit(self, slot: int, n: int, srs_offset: int = 0, partial: bool = False) -> Tuple[int, bool]:
        """Queue an MSM on a free lane and return its ticket; at most two tickets may be outstanding (E_BUSY)."""
        t = ctypes.c_int(-1)
        self._chk(self._lib.kzg_msm_submit(self._h, slot, n, srs_offset, int(partial), ctypes.byref(t)))
        return t.value, partial

    def msm_wait(self, ticket: Tuple[int, bool]) -> bytes:
        out = ctypes.create_string_buffer(192 if ticket[1] else 48)
        self._chk(self._lib.kzg_msm_wait(self._h, ticket[0], out))
        return out.raw

    def msm_cancel(self, ticket) -> None:
        """Give up an outstanding ticket (msm_submit / msm_sharded_begin): drains its lane and frees it."""
        self._chk(self._lib.kzg_msm_cancel(self._h, ticket[0] if isinstance(ticket, tuple) else ticket))

    def msm_partial_resident_dev(self, slot: int, n: int, srs_offset: int, dev_ptr: int) -> None:
        """The 192-byte partial goes to device address `dev_ptr` (e.g. `tensor.data_ptr()`); complete on return."""
        self._chk(self._lib.kzg_msm_partial_resident_dev(self._h, slot, n, srs_offset, ctypes.c_void_p(dev_ptr)))

    def g1_sum_dev(self, dev_ptr: int, count: int) -> bytes:
        """Sum of `count` partials at device address `dev_ptr` (every writer must have completed) -> 48 bytes."""
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_g1_sum_dev(self._h, ctypes.c_void_p(dev_ptr), count, out))
        return out.raw

    def msm_sharded_begin(self, slot: int, n: int, srs_offset: int, dev_ptr: int, consumer_stream: int) -> int:
        """Queue this rank's partial MSM; its 192 bytes land at `dev_ptr` and `consumer_stream` (a raw hipStream_t, e.g.
        `torch.cuda.current_stream().cuda_stream`) waits for them on the device.  Returns a ticket; nothing blocks."""
        t = ctypes.c_int(-1)
        self._chk(self._lib.kzg_msm_sharded_begin(self._h, slot, n, srs_offset, ctypes.c_void_p(dev_ptr),
                                                  ctypes.c_void_p(consumer_stream), ctypes.byref(t)))
        return t.value

    def msm_sharded_finish(self, ticket: int, dev_ptr: int, count: int, producer_stream: int) -> bytes:
        """Sum the `count` gathered partials at `dev_ptr` once `producer_stream` has reached this point -> 48 bytes."""
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_msm_sharded_finish(self._h, ticket, ctypes.c_void_p(dev_ptr), count,
                                                   ctypes.c_void_p(producer_stream), out))
        return out.raw

    # ------------------------------------------------------------------ the library's own collective (kzg_comm_*)
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId through the library: ONE rank calls it and hands the 128 bytes to the others (rendezvous is the
        caller's: a store, a file, a socket)."""
        lib = _native.load()
        out = ctypes.create_string_buffer(128)
        rc = lib.kzg_comm_unique_id(out)
        if rc != 0:
            raise KzgError(rc, lib.kzg_last_error(None).decode(errors="replace"))
        return out.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int, timeout_ms: int = 0, init_timeout_ms: int = 0) -> None:
        """Joins the `world`-rank RCCL communicator on this context's GPU (collective: returns when every rank has joined
        and a first checked all_gather has connected them).  `init_timeout_ms` > 0 bounds that rendezvous in the library
        (kzg_comm_init_bounded): peers that never arrive raise KzgError(E_COMM) and the engine stays usable.
        `timeout_ms` is the per-call budget of every later sharded MSM."""
        if len(unique_id) != 128:
            raise ValueError("the RCCL unique id is 128 bytes")
        self._chk(self._lib.kzg_comm_init_bounded(self._h, unique_id, rank, world, int(init_timeout_ms)))
        if timeout_ms:
            self._chk(self._lib.kzg_comm_set_timeout(self._h, timeout_ms))

    def comm_set_timeout(self, timeout_ms: int) -> None:
        self._chk(self._lib.kzg_comm_set_timeout(self._h, timeout_ms))

    def comm_selftest(self) -> None:
        """One small all_gather with checked content on the communicator (collective): raises KzgError(E_COMM) when the
        ranks cannot actually exchange bytes."""
        self._chk(self._lib.kzg_comm_selftest(self._h))

    def comm_destroy(self) -> None:
        self._chk(self._lib.kzg_comm_destroy(self._h))

    def comm_info(self) -> Dict[str, int]:
        arr = (ctypes.c_int32 * 4)()
        self._chk(self._lib.kzg_comm_info(self._h, arr))
        v = int(arr[2])
        return {"rank": arr[0], "world": arr[1], "rccl_version_code": v, "broken": bool(arr[3]),
                "rccl_version": f"{v // 10000}.{v // 100 % 100}.{v % 100}" if v else None}

    def msm_sharded(self, slot: int, n: int, srs_offset: int = 0) -> bytes:
        """This rank's SRS segment -> partial -> ncclAllGather on the lane's own stream -> sum: 48 bytes, the same on
        every rank.  One host wait; nothing but the library between the partial and the sum."""
        out = ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_msm_sharded(self._h, slot, n, srs_offset, out))
        return out.raw

    def commit_open_resident(self, i: int, slot: int, T: int, alpha_be32: bytes,
                             evaluation_form: bool = True) -> Tuple[bytes, bytes, bytes]:
        c, ev, pf = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        self._chk(self._lib.kzg_commit_open_resident(self._h, i, slot, T, int(evaluation_form), alpha_be32, c, ev, pf))
        return c.raw, ev.raw, pf.raw

    def ntt_resident(self, slot: int, n: int, inverse: bool) -> None:
        self._chk(self._lib.kzg_ntt_resident(self._h, slot, n, int(inverse)))

    # ------------------------------------------------------------------ measurement
    def set_profiling(self, level) -> None:
        """0 / False: off.  1 / True: HIP events around every stage (calls serialise on one lane).  2: around the
        accumulate kernel only (two events per launch, no serialisation)."""
        self._chk(self._lib.kzg_set_profiling(self._h, int(level)))

    def timings(self) -> Dict[str, float]:
        arr = (ctypes.c_float * len(_native.TIMING_NAMES))()
        self._chk(self._lib.kzg_get_timings(self._h, arr, len(arr)))
        return {k: float(v) for k, v in zip(_native.TIMING_NAMES, arr)}

    def msm_plan(self, n: int) -> Dict[str, int]:
        arr = (ctypes.c_int32 * 4)()
        self._chk(self._lib.kzg_msm_plan(self._h, n, arr))
        return {"chunk": arr[0], "lanes": arr[1], "buckets": arr[2], "windows": arr[3]}

    def calibrate(self, waves_per_simd: int = 2) -> Dict[str, float]:
        """The v_mad_u64_u32 issue rate of THIS GPU right now (kzg_calibrate): what bounds k_msm_accumulate."""
        arr = (ctypes.c_double * 6)()
        self._chk(self._lib.kzg_calibrate(self._h, waves_per_simd, arr))
        return {"ns_per_mad_per_simd": arr[0], "gmad_per_s": arr[1], "memtime_ticks_per_ns": arr[2], "kernel_ms": arr[3],
                "simds": int(arr[4]), "ticks_per_mad_of_one_wave": arr[5], "waves_per_simd": waves_per_simd}

    # ------------------------------------------------------------------ unit-op hooks (parity tests)
    def test_field(self, field: int, op: int, a_be: bytes, b_be: bytes) -> bytes:
        w = 48 if field == 0 else 32
        out = ctypes.create_string_buffer(len(a_be))
        self._chk(self._lib.kzg_test_field(self._h, field, op, a_be, b_be, out, len(a_be) // w))
        return out.raw

    def test_fr_inv(self, in_be32: bytes) -> Tuple[bytes, List[int]]:
        """The device-side Fr inversion alone (kzg_test_field, Fr ops 7 and 8): (inverses as n x 32 bytes, zero flags)."""
        flags = self.test_field(1, 8, in_be32, in_be32)
        return self.test_field(1, 7, in_be32, in_be32), [flags[32 * j + 31] for j in range(len(in_be32) // 32)]

    def test_fr_batch_inv(self, in_be32: bytes) -> bytes:
        """The batched inversion of commit_lookup_sum alone (kzg_test_field, Fr op 9): the n inverses as n x 32 bytes;
        KzgError(KZG_E_ARG) when an element is zero."""
        return self.test_field(1, 9, in_be32, in_be32)

    def test_g1(self, op: int, a_be96: bytes, b_be96: bytes) -> bytes:
        out = ctypes.create_string_buffer(len(a_be96))
        self._chk(self._lib.kzg_test_g1(self._h, op, a_be96, b_be96, out, len(a_be96) // 96))
        return out.raw

    def test_fp_raw(self, field: int, op: int, *operands) -> List[List[int]]:
        """One field operation on raw working limbs (kzg_test_fp_raw): up to four operands, each a list of n elements of 14
        (field 0, Fp) or 9 (field 1, Fr) limbs; the n results, limbs as they leave the operation."""
        w = 14 if field == 0 else 9
        n = len(operands[0])
        arrs = []
        for elems in operands:
            flat = [x for e in elems for x in e]
            if len(elems) != n or len(flat) != n * w:
                raise ValueError(f"raw operands must be {n} elements of {w} limbs")
            arrs.append((ctypes.c_uint32 * (n * w))(*flat))
        arrs += [None] * (4 - len(arrs))
        out = (ctypes.c_uint32 * (n * w))()
        self._chk(self._lib.kzg_test_fp_raw(self._h, field, op, *arrs, out, n))
        out = list(out)
        return [out[w * j:w * j + w] for j in range(n)]

    def test_g1_raw(self, op: int, a_xyzz: List[List[int]], b_xyzz: List[List[int]] = None) -> bytes:
        """One point operation on raw XYZZ limbs (kzg_test_g1_raw): n operands of 56 limbs each; n affine points x 96 bytes."""
        n = len(a_xyzz)
        arrs = []
        for pts in (a_xyzz, b_xyzz):
            if pts is None:
                arrs.append(None)
                continue
            flat = [x for e in pts for x in e]
            if len(flat) != n * 56:
                raise ValueError(f"raw points must be {n} records of 56 limbs")
            arrs.append((ctypes.c_uint32 * (n * 56))(*flat))
        out = ctypes.create_string_buffer(96 * n)
        self._chk(self._lib.kzg_test_g1_raw(self._h, op, arrs[0], arrs[1], out, n))
        return out.raw

    def test_ntt_run(self, vals_be32: bytes, inverse: bool, kernel: int, S: Sequence[int], logC: Sequence[int]) -> bytes:
        """The transform of 2^log_n elements by the CALLER'S pass plan (kzg_test_ntt_run): kernel 0 register-blocked, 1 radix-2;
        pass p runs S[p] stages on tiles of 2^logC[p] columns.  KzgError(KZG_E_ARG) for a plan the kernels do not admit."""
        n = len(vals_be32) // 32
        if n < 2 or n & (n - 1) or len(S) != len(logC):
            raise KzgError(_native.KZG_E_ARG, "ntt plan: 2^log_n elements with log_n >= 1, one logC per S")
        buf = ctypes.create_string_buffer(vals_be32, len(vals_be32))
        arr_s, arr_c = (ctypes.c_int * max(1, len(S)))(*S), (ctypes.c_int * max(1, len(S)))(*logC)
        self._chk(self._lib.kzg_test_ntt_run(self._h, ctypes.addressof(buf), n.bit_length() - 1, int(inverse), kernel, len(S),
                                             arr_s, arr_c))
        return buf.raw

    def test_poly_run(self, form: int, f_be32: bytes, n: int, alphas_be32: bytes, plan: Sequence[int] = (-1, -1, -1, -1),
                      rows: int = 1, pairs: Sequence[Tuple[int, int]] = (), pts: Optional[Sequence[int]] = None,
                      f_mont: bool = False) -> Tuple[bytes, bytes]:
        """The opening scan of rows x n coefficients by the CALLER'S plan (kzg_test_poly_run; no SRS, no MSM): plan = (l0,
        scan_max, scan_nt, lds), all -1 for the library's own.  form 0 open (alpha as kernel argument), 1 evaluate (alpha from
        memory), 2 rows side by side, 3 (row, point) pairs, 4 vectors at their points, 5 the chained division (vector p at point
        pts[p], Montgomery quotients).  Returns (the evaluations, 32 bytes each; the raw quotient buffer of rows x n x 8
        little-endian words, empty for forms 1 - 3).  KzgError(KZG_E_ARG) for a plan the kernels do not admit."""
        l0, scan_max, scan_nt, lds = plan
        nout = len(pairs) if form == 3 else rows
        y = ctypes.create_string_buffer(32 * max(1, nout))
        quot = form in (0, 4, 5)
        q = (ctypes.c_uint32 * (8 * rows * n))() if quot else None
        pr, pp = bytes(r for r, _ in pairs), bytes(p for _, p in pairs)
        self._chk(self._lib.kzg_test_poly_run(self._h, form, l0, scan_max, scan_nt, lds, f_be32, n, rows, int(f_mont), pr, pp,
                                              len(pairs), bytes(pts) if pts is not None else None, alphas_be32,
                                              len(alphas_be32) // 32, ctypes.addressof(y), ctypes.addressof(q) if quot else None))
        return y.raw[:32 * nout], bytes(q) if quot else b""

    def test_recur_run(self, a_be32: bytes, b_be32: bytes, start_be32: bytes, n: int,
                       plan: Sequence[int] = (-1, -1)) -> Tuple[bytes, bytes]:
        """v[0] = start, v[t + 1] = a[t] v[t] + b[t] over n steps by the CALLER'S plan (kzg_test_recur_run; no SRS, no MSM): plan =
        (l0, top_max), both -1 for the library's own.  Returns (v[0] .. v[n - 1] as n x 32 bytes, the closing value v[n]).
        KzgError(KZG_E_ARG) for a plan the kernels do not admit."""
        l0, top_max = plan
        v, cl = ctypes.create_string_buffer(32 * max(1, n)), ctypes.create_string_buffer(32)
        self._chk(self._lib.kzg_test_recur_run(self._h, l0, top_max, a_be32, b_be32, start_be32, n, ctypes.addressof(v),
                                               ctypes.addressof(cl)))
        return v.raw[:32 * n], cl.raw

    def test_scan_run(self, form: int, a_be32: bytes, b_be32: Optional[bytes], start_be32: Optional[bytes], n: int,
                      plan: Sequence[int] = (-1, -1)) -> Tuple[bytes, bytes, int]:
        """The product scan or the additive scan over n elements by the CALLER'S plan (kzg_test_scan_run; no SRS, no MSM): plan =
        (l0, top_max), both -1 for the library's own.  form 0: out[t] = prod_{u<t} a[u] / b[u] (launch_gp_scan); 1: the same times
        start; 2: 1 / a[t] (launch_fr_batch_inv, out = W); 3: b[t] / a[t] (launch_fr_batch_inv, out = P); 4: sum_{u<t} a[u]
        (launch_lk_sum_scan).  Returns (out as n x 32 bytes, the closing value, the zero-denominator flag word).
        KzgError(KZG_E_ARG) for a plan the kernels do not admit."""
        l0, top_max = plan
        v, cl, zf = ctypes.create_string_buffer(32 * max(1, n)), ctypes.create_string_buffer(32), ctypes.c_uint32(0)
        self._chk(self._lib.kzg_test_scan_run(self._h, form, l0, top_max, a_be32, b_be32, start_be32, n, ctypes.addressof(v),
                                              ctypes.addressof(cl), ctypes.byref(zf)))
        return v.raw[:32 * n], cl.raw, zf.value

    def test_join(self, build: int, walk: int, tab_be32: bytes, in_be32: bytes, T: int, rows: int, w: int, cap: int,
                  n_pay: int = 0, index: bool = False, sel_be32: Optional[bytes] = None) -> Dict[str, object]:
        """The hash join alone through the library's own launchers at the CALLER'S capacity (kzg_test_join; no SRS, no MSM):
        build 0 launch_join_build, 1 _build_rows; walk 0 launch_join_probe, 1 _probe_rows, 2 _probe_sel (sel_be32: the selector
        column), 3 launch_join_fetch.  tab_be32: (w + n_pay) x T canonical cells, column-major; in_be32: w x T.  Returns {"slots":
        the cap slot words (2^32 - 1: empty), "home_tab", "home_in": the T home slots of the table rows and of the cells, "cnt":
        the T counters, "fetched": the index + n_pay fetched columns as bytes (walk 3), "missing", "first" (None: no miss),
        "overrun"}.  KzgError(KZG_E_ARG) for arguments outside the kernels' preconditions."""
        if len(tab_be32) != 32 * (w + n_pay) * T or len(in_be32) != 32 * w * T or (sel_be32 is not None and len(sel_be32) != 32 * T):
            raise KzgError(_native.KZG_E_ARG, "join: (w + n_pay) x T table cells, w x T input cells, T selector cells")
        n_out = n_pay + int(index) if walk == 3 else 0
        slots, home = (ctypes.c_uint32 * max(1, cap))(), (ctypes.c_uint32 * max(1, 2 * T))()
        cnt, fetched = (ctypes.c_uint32 * max(1, T))(), ctypes.create_string_buffer(32 * max(1, n_out * T))
        missing, first, overrun = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._chk(self._lib.kzg_test_join(self._h, build, walk, tab_be32, in_be32, sel_be32, T, rows, w, n_pay, int(index), cap,
                                          ctypes.addressof(slots), ctypes.addressof(home), ctypes.addressof(cnt),
                                          ctypes.addressof(fetched), ctypes.byref(missing), ctypes.byref(first),
                                          ctypes.byref(overrun)))
        home = list(home)
        return {"slots": list(slots), "home_tab": home[:T], "home_in": home[T:], "cnt": list(cnt),
                "fetched": [fetched.raw[32 * T * c:32 * T * (c + 1)] for c in range(n_out)], "missing": missing.value,
                "first": None if first.value == (1 << 64) - 1 else first.value, "overrun": overrun.value}

    def test_join_counts(self, counters: Sequence[int]) -> bytes:
        """launch_join_counts over caller-given counter words (kzg_test_join_counts): 32 canonical big-endian bytes each."""
        n = len(counters)
        out = ctypes.create_string_buffer(32 * max(1, n))
        self._chk(self._lib.kzg_test_join_counts(self._h, (ctypes.c_uint32 * max(1, n))(*counters), n, ctypes.addressof(out)))
        return out.raw[:32 * n]


def ntt_plan_of(log_n: int, kernel: int = -1, tile_log: int = 0) -> Tuple[int, List[Tuple[int, int]]]:
    """The pass plan the library runs for 2^log_n elements (kzg_test_ntt_plan_of; no context, no device): (form, [(S, logC)
    per pass]) with form 0 register-blocked / 1 radix-2.  kernel -1: the library's choice, 0 / 1: that form; tile_log 0: the
    library's tile, 8 .. 11: that tile."""
    lib = _native.load()
    arr_s, arr_c, passes = (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), ctypes.c_int(0)
    form = lib.kzg_test_ntt_plan_of(log_n, kernel, tile_log, arr_s, arr_c, ctypes.byref(passes))
    if form < 0:
        raise KzgError(form, lib.kzg_last_error(None).decode(errors="replace"))
    return form, [(arr_s[p], arr_c[p]) for p in range(passes.value)]


def poly_plan_of(n: int, l0: int = -1, scan_max: int = -1, scan_nt: int = -1, lds: int = -1) -> Dict[str, object]:
    """The level plan of the opening scan for n coefficients (kzg_test_poly_plan_of; no context, no device): with every
    parameter -1 the plan the library runs, otherwise the caller's.  {"K", "l", "sq", "n", "off" (K + 1 entries each), "scan_nt",
    "lds"}; KzgError(KZG_E_ARG) with the reason for a plan outside the kernels' preconditions."""
    lib = _native.load()
    K, nt, ld = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    al, asq, an, aoff = (ctypes.c_int * 16)(), (ctypes.c_int * 16)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    rc = lib.kzg_test_poly_plan_of(n, l0, scan_max, scan_nt, lds, ctypes.byref(K), al, asq, an, aoff, ctypes.byref(nt),
                                   ctypes.byref(ld))
    if rc != _native.KZG_OK:
        raise KzgError(rc, lib.kzg_last_error(None).decode(errors="replace"))
    k = K.value + 1
    return {"K": K.value, "l": list(al[:k]), "sq": list(asq[:k]), "n": list(an[:k]), "off": list(aoff[:k]), "scan_nt": nt.value,
            "lds": ld.value}


def recur_plan_of(n: int, l0: int = -1, top_max: int = -1) -> Dict[str, object]:
    """The level plan of the recurrence scan for n steps (kzg_test_recur_plan_of; no context, no device): with both parameters
    -1 the plan the library runs, otherwise the caller's.  {"K", "l", "n", "off" (K + 1 entries each)}; KzgError(KZG_E_ARG) with
    the reason for a plan outside the kernels' preconditions."""
    lib = _native.load()
    K = ctypes.c_int(0)
    al, an, aoff = (ctypes.c_int * 16)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    rc = lib.kzg_test_recur_plan_of(n, l0, top_max, ctypes.byref(K), al, an, aoff)
    if rc != _native.KZG_OK:
        raise KzgError(rc, lib.kzg_last_error(None).decode(errors="replace"))
    k = K.value + 1
    return {"K": K.value, "l": list(al[:k]), "n": list(an[:k]), "off": list(aoff[:k])}


def scan_plan_of(n: int, l0: int = -1, top_max: int = -1) -> Dict[str, object]:
    """The level plan of the product scan and of the additive scan for n elements (kzg_test_scan_plan_of; no context, no
    device): with both parameters -1 the plan the library runs, otherwise the caller's.  {"K", "l", "n", "off" (K + 1 entries
    each)}, K >= 1; KzgError(KZG_E_ARG) with the reason for a plan outside the kernels' preconditions."""
    lib = _native.load()
    K = ctypes.c_int(0)
    al, an, aoff = (ctypes.c_int * 16)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    rc = lib.kzg_test_scan_plan_of(n, l0, top_max, ctypes.byref(K), al, an, aoff)
    if rc != _native.KZG_OK:
        raise KzgError(rc, lib.kzg_last_error(None).decode(errors="replace"))
    k = K.value + 1
    return {"K": K.value, "l": list(al[:k]), "n": list(an[:k]), "off": list(aoff[:k])}


def msm_passes_of(c: int, long_rows: bool, k: int, m: int) -> List[Tuple[int, int, int, int, int]]:
    """The MSM passes the library runs for a multi-row call's k row sets + m tail sets (the openings' quotients) at window c
    (kzg_test_msm_passes; no context, no device): per pass (first row, rows, first tail set, tail sets, lane)."""
    lib = _native.load()
    out, passes = (ctypes.c_uint32 * (5 * max(1, k + m)))(), ctypes.c_int(0)
    rc = lib.kzg_test_msm_passes(c, int(long_rows), k, m, out, ctypes.byref(passes))
    if rc != _native.KZG_OK:
        raise KzgError(rc, lib.kzg_last_error(None).decode(errors="replace"))
    return [tuple(out[5 * p:5 * p + 5]) for p in range(passes.value)]


class RowSet:
    """Rows committed by HipEngine.commit_rows and kept on the device: `handle`, worker `i`, `k` rows of `T` elements and
    their `commitments` (48-byte compressed G1 each).  release() frees the device copy; a `with` block releases on exit."""

    def __init__(self, engine, handle: int, i: int, k: int, T: int, commitments: List[bytes]):
        self.engine, self.handle, self.i, self.k, self.T = engine, handle, i, k, T
        if T is not None and hasattr(engine, "_set_len"):
            engine._set_len[int(handle)] = (i, T)   # what a _zk builder needs when it is handed the bare handle
        if hasattr(engine, "_set_rows"):
            engine._set_rows[int(handle)] = k
        self.commitments = commitments
        self.released = False

    def release(self) -> None:
        if not self.released:
            self.released = True
            self.engine.release_rows(self.handle)

    def __enter__(self) -> "RowSet":
        return self

    def __exit__(self, *exc) -> bool:
        self.release()
        return False

    def __repr__(self) -> str:
        return f"RowSet(handle={self.handle}, i={self.i}, k={self.k}, T={self.T})"


class QuotientAcc:
    """The accumulator of HipEngine.quotient_part: `handle`, worker `i`, row length `T` and `ext_log` of a device vector of
    T << ext_log field elements.  Not a row set: only quotient_part and quotient_finish take it.  release() frees it (a
    finished accumulator is consumed and needs none); a `with` block releases on exit."""

    def __init__(self, engine, handle: int, i: int, T: int, ext_log: int):
        self.engine, self.handle, self.i, self.T, self.ext_log = engine, handle, i, T, ext_log
        self.released = False

    def release(self) -> None:
        if not self.released:
            self.released = True
            self.engine.release_rows(self.handle)

    def __enter__(self) -> "QuotientAcc":
        return self

    def __exit__(self, *exc) -> bool:
        self.release()
        return False

    def __repr__(self) -> str:
        return f"QuotientAcc(handle={self.handle}, i={self.i}, T={self.T}, ext_log={self.ext_log})"
