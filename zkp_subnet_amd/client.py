"""`Client`: same method surface as the `fourier.Client` the reference miner / validator drive
(construction: reference base/miner.py:73-84, base/validator.py:80-91; calls: neurons/miner.py:39,48 and
neurons/validator.py:59-104), backed by the in-process HIP library instead of a spawned Rust binary over
localhost HTTP.  Every method returns a `Response` usable exactly like the reference uses the HTTP one:

    with client.worker_commit(i, poly) as response:
        if response.status_code != 200: ...
        response.json().get("commitment")

Errors never escape as exceptions (the reference checks status_code, neurons/miner.py:40-44): bad input -> 400,
prover failure -> 500, not implemented -> 501.
"""
from __future__ import annotations

import logging
import os
import secrets
import struct
from typing import Any, Dict, List, Optional, Sequence

from . import codec
from ._native import (COL_DTYPES, COL_KINDS, KZG_E_ARG, KZG_E_POINT, KZG_E_SCALAR, KZG_MAX_BATCH_OPEN, KZG_MAX_OPEN_POINTS, KZG_MAX_SHPLONK_POINTS,
                      KZG_MAX_SHPLONK_ROWS, KzgError, open_masks, shplonk_masks)

R_MODULUS = codec.R_MODULUS
log = logging.getLogger("zkp_subnet_amd.client")


class Response:
    """Minimal stand-in for the HTTP response object of the reference client."""

    def __init__(self, status_code: int, body: Optional[Dict[str, Any]] = None):
        self.status_code = status_code
        self._body = body or {}

    def json(self) -> Dict[str, Any]:
        return self._body

    def __enter__(self) -> "Response":
        return self

    def __exit__(self, *exc) -> bool:
        return False

    def close(self) -> None:
        pass


def _guard(fn):
    def wrapped(self, *a, **kw):
        try:
            if self.engine is None:
                return Response(503, {"error": "prover not started"})
            return Response(200, fn(self, *a, **kw))
        except codec.CodecError as e:
            return Response(400, {"error": str(e)})
        except KzgError as e:
            bad_input = e.code in (KZG_E_ARG, KZG_E_SCALAR, KZG_E_POINT)
            return Response(400 if bad_input else 500, {"error": str(e)})
        except NotImplementedError as e:
            return Response(501, {"error": str(e)})
        except Exception as e:  # never let the axon thread die (reference neurons/miner.py:133-135)
            return Response(500, {"error": f"{type(e).__name__}: {e}"})

    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


_NO_PARAMS = object()   # _unit_objects: the request has no params object (None is a params a caller may send)


def _handles(handles) -> List[int]:
    """committed-row-set handles from a request: 1 .. 16 non-negative integers"""
    try:
        hs = [int(h) for h in handles]
    except (TypeError, ValueError) as e:
        raise codec.CodecError(f"row-set handles must be integers: {e}") from e
    if not 1 <= len(hs) <= KZG_MAX_BATCH_OPEN or any(h < 0 or h >= 1 << 64 for h in hs):
        raise codec.CodecError(f"{len(hs)} row-set handles, expected 1 .. {KZG_MAX_BATCH_OPEN} values in [0, 2^64)")
    return hs


class Client:
    """Drop-in for fourier.Client.  `port` and `bin` are accepted and ignored (there is no child process);
    `setup_path` names a file holding the 2^scale-point SRS as uncompressed affine G1 points (x||y, 96 B each,
    big-endian) or, with `uncompressed=False`, as 48-byte ZCash-compressed points (decompressed on the GPU).
    A missing setup file is an error, as it is for the reference prover.  A synthetic tau-derived SRS (generated on
    the GPU; its trapdoor is a public function of `seed`, so openings against it can be forged by anyone) is only
    built on explicit request -- `synthetic=True` or an explicit `seed` -- for tests and benches (mirrors
    `fourier setup --generate-setup`, reference tests/conftest.py:50-65), and is logged loudly."""

    def __init__(self, port: int = 1337, bin: str = "", uncompressed: bool = True, setup_path: str = "",
                 precompute_path: str = "", engine: Any = None, device: int = 0, seed: Optional[int] = None,
                 workers: Optional[Sequence[int]] = None, synthetic: Optional[bool] = None):
        self.port, self.bin, self.uncompressed = port, bin, uncompressed
        self.setup_path, self.precompute_path = setup_path, precompute_path
        self.engine = engine
        self._own_engine = engine is None
        self.device = device
        self.seed = seed
        self.synthetic = (seed is not None) if synthetic is None else bool(synthetic)
        self.workers = list(workers) if workers is not None else None
        self.scale = self.machines_scale = 0
        self._accs: Dict[int, Any] = {}   # live quotient accumulators made through worker_quotient_part, by handle

    # ------------------------------------------------------------------ lifecycle (base/miner.py:82-84,155,181)
    def start(self, scale: int = 18, machines_scale: int = 8) -> None:
        if scale < machines_scale:
            raise ValueError("scale must be >= machines_scale")
        self.scale, self.machines_scale = scale, machines_scale
        if self.engine is None:
            from .engine import HipEngine  # raises loudly without the HIP library / a gfx950 device

            self.engine = HipEngine(self.device)
            info = self.engine.runtime_info()
            if 0 < info["lanes_concurrent"] < info["lanes"]:
                log.warning("only %d of the context's %d lanes run concurrently on this GPU (GPU_MAX_HW_QUEUES=%s%s): results "
                            "are unaffected, but concurrent requests overlap less.  Export GPU_MAX_HW_QUEUES=8 before the "
                            "process's first HIP call.", info["lanes_concurrent"], info["lanes"],
                            info["hw_queues_env"] or "unset", ", HIP was already initialised when the library was loaded"
                            if info["hip_live_at_load"] else "")
        if self.setup_path and os.path.exists(self.setup_path):
            rec = 96 if self.uncompressed else 48      # the reference's `uncompressed` flag (base/miner.py:77)
            if os.path.getsize(self.setup_path) % rec:
                raise ValueError(f"setup file must be a whole number of {rec}-byte G1 points "
                                 f"(uncompressed={self.uncompressed})")
            rec_points = os.path.getsize(self.setup_path) // rec
            T = 1 << (scale - machines_scale)
            file_slices = rec_points // T if rec_points % T == 0 else 0
            # a client that serves only SOME worker indices (one device of a MultiDeviceClient: i = g mod G) loads only their
            # slices when they form the progression first, first + stride, ... over the file's slices
            if self.workers is not None and not self.workers:      # more devices than worker rows: this one serves none
                self._slice_of = {}
                return
            prog = self._progression(file_slices) if self.workers is not None else None
            load_slices = getattr(self.engine, "load_srs_file_slices", None)
            load_file = getattr(self.engine, "load_srs_file", None)
            if prog is not None and load_slices is not None:
                load_slices(self.setup_path, scale, machines_scale, prog[0], prog[1], compressed=not self.uncompressed)
                self._slice_of = {w: k for k, w in enumerate(self.workers)}
            elif load_file is not None:                # HipEngine: the library reads the file and streams it itself
                load_file(self.setup_path, scale, machines_scale, compressed=not self.uncompressed)
                self._slice_of = None
            else:                                      # an injected engine without a file loader (tests)
                with open(self.setup_path, "rb") as f:
                    self.engine.load_srs(f.read(), scale, machines_scale, compressed=not self.uncompressed)
                self._slice_of = None
            vk_path = self.setup_path + ".vk"   # 192 B [tau_x]_2 (uncompressed) + one 96 B [L_i(tau_y)]_1 per slice
            if os.path.exists(vk_path) and hasattr(self.engine, "set_verifier_key"):
                with open(vk_path, "rb") as f:
                    vk = f.read()
                li = vk[192:]
                if self._slice_of is not None:         # the key's factors in RESIDENT slice order
                    li = b"".join(li[96 * w:96 * w + 96] for w in self.workers)
                self.engine.set_verifier_key(vk[:192], li)
        else:
            if not self.synthetic:
                if self._own_engine:
                    self.engine.close()
                    self.engine = None
                raise FileNotFoundError(
                    f"setup file {self.setup_path!r} not found: generate one with `python -m zkp_subnet_amd.setup_cli "
                    "setup --generate-setup ...`.  A synthetic SRS (public trapdoor: forgeable openings) is only built "
                    "when asked for with Client(synthetic=True) or an explicit seed (tests / benches).")
            seed = self.seed if self.seed is not None else 0
            log.warning("SYNTHETIC SRS from public seed %d: its trapdoor is computable by anyone -- openings can be "
                        "forged.  Tests and benches only; production needs a setup file (setup_path).", seed)
            tau_x, tau_y = derive_taus(seed)
            self.tau_x, self.tau_y = tau_x, tau_y
            if self.workers is not None and not self.workers:
                # a device of a MultiDeviceClient with MORE devices than worker rows serves no row: nothing to generate, and
                # every worker index answers "no resident slice" (400) here
                self._slice_of = {}
                return
            self.engine.gen_srs(tau_x, tau_y, scale, machines_scale, self.workers)
            self._slice_of = {w: k for k, w in enumerate(self.workers)} if self.workers is not None else None

    def _progression(self, file_slices: int):
        """(first, stride) when self.workers is exactly first, first + stride, ... below file_slices; else None."""
        w = self.workers
        if not w or file_slices <= 0:
            return None
        first = w[0]
        stride = (w[1] - w[0]) if len(w) > 1 else max(1, file_slices)
        if stride <= 0 or list(w) != list(range(first, file_slices, stride)):
            return None
        return first, stride

    def stop(self) -> None:
        if self.engine is not None and self._own_engine:
            self.engine.close()
        if self._own_engine:
            self.engine = None

    def _slice(self, i: int) -> int:
        i = int(i)
        if i < 0 or i >= (1 << self.machines_scale):
            raise codec.CodecError(f"worker index {i} outside [0, 2^{self.machines_scale})")
        if self._slice_of is not None:
            if i not in self._slice_of:
                raise codec.CodecError(f"worker index {i} has no resident SRS slice")
            return self._slice_of[i]
        return i

    # ------------------------------------------------------------------ miner side (neurons/miner.py:38-61)
    @_guard
    def worker_commit(self, i: int, poly: Sequence[str]):
        fast = getattr(self.engine, "commit_list", None)      # HipEngine: text decoded straight into pinned staging
        c = fast(self._slice(i), poly, True) if fast and codec._wire else \
            self.engine.commit(self._slice(i), codec.fr_list_to_be32(poly), True)
        return {"commitment": codec.g1_to_b64(c)}

    @_guard
    def worker_open(self, i: int, poly: Sequence[str], x: str):
        fast = getattr(self.engine, "open_list", None)
        ev, pf = fast(self._slice(i), poly, codec.fr_to_be32(x), True) if fast and codec._wire else \
            self.engine.open(self._slice(i), codec.fr_list_to_be32(poly), codec.fr_to_be32(x), True)
        return {"eval": codec.be32_to_fr(ev), "proof": codec.g1_to_b64(pf)}

    @_guard
    def worker_commit_and_open(self, i: int, poly: Sequence[str], x: str):
        """Fused extension (one upload, one IFFT): what Miner.rpc_commit_and_open needs (neurons/miner.py:56-61)."""
        fast = getattr(self.engine, "commit_open_list", None)
        c, ev, pf = fast(self._slice(i), poly, codec.fr_to_be32(x), True) if fast and codec._wire else \
            self.engine.commit_open(self._slice(i), codec.fr_list_to_be32(poly), codec.fr_to_be32(x), True)
        return {"commitment": codec.g1_to_b64(c), "eval": codec.be32_to_fr(ev), "proof": codec.g1_to_b64(pf)}

    @_guard
    def worker_commit_open_batch(self, i: int, polys: Sequence[Sequence[str]], x: str, gamma: str):
        """Extension: k rows of worker i (a PLONK sub-circuit's wires, permutation and quotient pieces) opened at x with
        ONE proof for sum_j gamma^j f_j.  gamma must be drawn by the verifier after the commitments are fixed."""
        k = len(polys)
        if k == 0 or k > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"worker_commit_open_batch: {k} rows, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        if any(len(p) != len(polys[0]) for p in polys):
            raise codec.CodecError("worker_commit_open_batch: rows of unequal length")
        a, g = codec.fr_to_be32(x), codec.fr_to_be32(gamma)
        fast = getattr(self.engine, "commit_open_batch_list", None)
        cs, evs, pf = fast(self._slice(i), polys, a, g, True) if fast and codec._wire else \
            self.engine.commit_open_batch(self._slice(i), [codec.fr_list_to_be32(p) for p in polys], a, g, True)
        return {"commitments": [codec.g1_to_b64(c) for c in cs], "evals": [codec.be32_to_fr(e) for e in evs],
                "proof": codec.g1_to_b64(pf)}

    @_guard
    def worker_commit_open_multi(self, i: int, polys: Sequence[Sequence[str]], points: Sequence[str],
                                 opened: Sequence[Sequence[int]], gammas: Sequence[str]):
        """Extension: k rows of worker i opened at m <= 4 points (a PLONK opening step: every row at zeta, the permutation
        accumulator also at zeta * omega), one proof per point for sum_t gamma_p^t f_{j_t} over opened[p].  The points and
        gammas must be drawn by the verifier after the commitments are fixed."""
        k, m = len(polys), len(points)
        if k == 0 or k > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"worker_commit_open_multi: {k} rows, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        if m == 0 or m > KZG_MAX_OPEN_POINTS or len(opened) != m or len(gammas) != m:
            raise codec.CodecError(f"worker_commit_open_multi: {m} points, {len(opened)} row lists, {len(gammas)} gammas")
        if any(len(p) != len(polys[0]) for p in polys):
            raise codec.CodecError("worker_commit_open_multi: rows of unequal length")
        a, g = [codec.fr_to_be32(x) for x in points], [codec.fr_to_be32(x) for x in gammas]
        fast = getattr(self.engine, "commit_open_multi_list", None)
        cs, evs, pfs = fast(self._slice(i), polys, a, opened, g, True) if fast and codec._wire else \
            self.engine.commit_open_multi(self._slice(i), [codec.fr_list_to_be32(p) for p in polys], a, opened, g, True)
        return {"commitments": [codec.g1_to_b64(c) for c in cs], "evals": [[codec.be32_to_fr(e) for e in ev] for ev in evs],
                "proofs": [codec.g1_to_b64(pf) for pf in pfs]}

    @_guard
    def worker_commit_rows(self, i: int, polys: Sequence[Sequence[str]]):
        """Extension: k <= 16 rows of worker i committed and kept on the device as one committed row set.  Returns the set's
        handle and the k commitments; worker_open_rows opens the set later, after the caller has fixed (and hashed) the
        commitments, and worker_release_rows frees it."""
        k = len(polys)
        if k == 0 or k > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"worker_commit_rows: {k} rows, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        if any(len(p) != len(polys[0]) for p in polys):
            raise codec.CodecError("worker_commit_rows: rows of unequal length")
        rs = self.engine.commit_rows(self._slice(i), [codec.fr_list_to_be32(p) for p in polys], True)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @_guard
    def worker_commit_rows_typed(self, i: int, columns: Sequence[object], fills: Optional[Sequence[Optional[str]]] = None,
                                 T: Optional[int] = None):
        """Extension: worker_commit_rows whose columns arrive as integers of their natural width.  A column is a C-contiguous
        one-dimensional buffer of u8, u16, u32, u64, i32 or i64 (a numpy array, an array.array), bytes of 32 big-endian bytes
        per cell, or the wire list of strings of worker_commit_rows, which goes through the codec as there: one call can mix
        an Fr column with typed ones.  T defaults to the longest column; a shorter column's cells behind its end take fills[c]
        (a wire string; null, or no fills at all: 0).  A negative cell x is r - |x|.  Returns what worker_commit_rows returns
        for the same values: the set is an ordinary one."""
        what = "worker_commit_rows_typed"
        k = len(columns)
        if k == 0 or k > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"{what}: {k} columns, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        if fills is not None and len(fills) != k:
            raise codec.CodecError(f"{what}: {len(fills)} fills for {k} columns (one each, or none at all)")
        if T is not None and (isinstance(T, bool) or not isinstance(T, int) or T < 1):
            raise codec.CodecError(f"{what}: T must be a positive integer or null")
        cols = []
        for c, col in enumerate(columns):
            if isinstance(col, (list, tuple)):
                col = codec.fr_list_to_be32(col)
            fill = None if fills is None or fills[c] is None else codec.fr_to_be32(fills[c])
            cols.append((col, fill))
        rs = self.engine.commit_rows_typed(self._slice(i), cols, True, T)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @_guard
    def worker_read_rows(self, handles: Sequence[int], row: int, first: int, count: int, dtype: str = "fr"):
        """Extension: cells [first, first + count) of row `row` of committed sets (rows numbered as in worker_open_rows), as
        the values on the domain: what was uploaded, or what a builder wrote.  dtype "fr" returns wire strings; "u8", "u16",
        "u32", "u64", "i32" and "i64" return Python integers, where a value >= r - 2^(w-1) reads as negative for the signed
        ones.  A cell that does not fit the dtype reads 0 and is counted: `overflow`, and `first_overflow`, the smallest such
        row index (null: none).  The sets are unchanged."""
        what = "worker_read_rows"
        hs = _handles(handles)
        if not isinstance(dtype, str) or dtype not in COL_DTYPES:
            raise codec.CodecError(f"{what}: dtype must be one of {sorted(COL_DTYPES)}")
        if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in (row, first, count)):
            raise codec.CodecError(f"{what}: row, first and count must be non-negative integers")
        kind = COL_DTYPES[dtype]
        raw, overflow, first_overflow = self.engine.read_rows(hs, row, first, count, kind, True)
        if dtype == "fr":
            cells = codec.be32_to_fr_list(raw)
        else:
            width, signed = COL_KINDS[kind]
            code = {1: "B", 2: "H", 4: "I", 8: "Q"}[width]
            cells = list(struct.unpack(f"<{count}{code.lower() if signed else code}", raw))
        return {"cells": cells, "overflow": int(overflow), "first_overflow": first_overflow}

    @_guard
    def worker_open_rows(self, handles: Sequence[int], points: Sequence[str], opened: Sequence[Sequence[int]],
                         gammas: Sequence[str]):
        """Extension: the rows of committed sets (numbered by concatenating the sets' rows in the order of `handles`)
        opened at m <= 4 points, one proof per point for sum_t gamma_p^t f_{j_t} over opened[p].  Equal to
        worker_commit_open_multi on the concatenated rows; worker_verify_open_multi checks it against the concatenated
        commitments."""
        hs = _handles(handles)
        m = len(points)
        if m == 0 or m > KZG_MAX_OPEN_POINTS or len(opened) != m or len(gammas) != m:
            raise codec.CodecError(f"worker_open_rows: {m} points, {len(opened)} row lists, {len(gammas)} gammas")
        open_masks(opened, KZG_MAX_BATCH_OPEN)   # the shape of `opened`; the engine checks it against the sets' rows
        a, g = [codec.fr_to_be32(x) for x in points], [codec.fr_to_be32(x) for x in gammas]
        evs, pfs = self.engine.open_rows(hs, a, opened, g)
        return {"evals": [[codec.be32_to_fr(e) for e in ev] for ev in evs], "proofs": [codec.g1_to_b64(pf) for pf in pfs]}

    @_guard
    def worker_eval_rows(self, handles: Sequence[int], points: Sequence[str], opened: Sequence[Sequence[int]]):
        """Extension: the evaluations of committed sets (rows numbered as in worker_open_rows) at m <= 4 points, no proof --
        what a Fiat-Shamir prover hashes before it derives the scalars of worker_open_rows_lincomb.  Equal to the evaluations
        worker_open_rows returns."""
        hs = _handles(handles)
        m = len(points)
        if m == 0 or m > KZG_MAX_OPEN_POINTS or len(opened) != m:
            raise codec.CodecError(f"worker_eval_rows: {m} points, {len(opened)} row lists")
        open_masks(opened, KZG_MAX_BATCH_OPEN)   # the shape of `opened`; the engine checks it against the sets' rows
        evs = self.engine.eval_rows(hs, [codec.fr_to_be32(x) for x in points], opened)
        return {"evals": [[codec.be32_to_fr(e) for e in ev] for ev in evs]}

    @_guard
    def worker_open_rows_lincomb(self, handles: Sequence[int], points: Sequence[str], coeffs: Sequence[Sequence[str]]):
        """Extension: one proof per point for h_p = sum_j coeffs[p][j] f_j over the k rows of committed sets (numbered as in
        worker_open_rows; coeffs[p] holds k scalars, a zero one leaves its row out).  Returns the values v_p = h_p(x_p) and
        the proofs; worker_verify_open_lincomb checks them against the sets' commitments."""
        hs = _handles(handles)
        m = len(points)
        if m == 0 or m > KZG_MAX_OPEN_POINTS or len(coeffs) != m:
            raise codec.CodecError(f"worker_open_rows_lincomb: {m} points, {len(coeffs)} coefficient lists")
        k = len(coeffs[0])
        if not 1 <= k <= KZG_MAX_BATCH_OPEN or any(len(c) != k for c in coeffs):
            raise codec.CodecError(f"worker_open_rows_lincomb: ragged coefficients, expected {m} lists of 1 .. "
                                   f"{KZG_MAX_BATCH_OPEN} scalars")
        vals, pfs = self.engine.open_rows_lincomb(hs, [codec.fr_to_be32(x) for x in points],
                                                  [[codec.fr_to_be32(c) for c in cs] for cs in coeffs])
        return {"values": [codec.be32_to_fr(v) for v in vals], "proofs": [codec.g1_to_b64(pf) for pf in pfs]}

    def _shplonk_args(self, what: str, points, opened, coeffs):
        """the shape checks the three SHPLONK text forms share; the decoded (points, coefficients)"""
        m, k = len(points), len(coeffs)
        if not 1 <= m <= KZG_MAX_SHPLONK_POINTS or len(opened) != m:
            raise codec.CodecError(f"{what}: {m} points, {len(opened)} row lists, expected 1 .. {KZG_MAX_SHPLONK_POINTS} of each")
        if not 1 <= k <= KZG_MAX_SHPLONK_ROWS:
            raise codec.CodecError(f"{what}: {k} coefficients, expected 1 .. {KZG_MAX_SHPLONK_ROWS}")
        try:
            shplonk_masks(opened, k)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: opened must hold lists of row indices: {e!r}") from e
        return [codec.fr_to_be32(x) for x in points], [codec.fr_to_be32(c) for c in coeffs]

    @_guard
    def worker_commit_shplonk(self, handles: Sequence[int], points: Sequence[str], opened: Sequence[Sequence[int]],
                              coeffs: Sequence[str]):
        """Extension: round A of a SHPLONK opening over the rows of committed sets (numbered as in worker_open_rows): opened[p]
        lists the rows opened at point p (up to 8 distinct points), coeffs holds one scalar per row.  h is computed and
        committed on the device as a new one-row set; returns its handle and W, its commitment.  The coefficients must be
        drawn after the commitments and the evaluations of worker_eval_rows are fixed."""
        hs = _handles(handles)
        a, c = self._shplonk_args("worker_commit_shplonk", points, opened, coeffs)
        w, rs = self.engine.commit_shplonk(hs, a, opened, c)
        return {"handle": int(rs.handle), "w": codec.g1_to_b64(w)}

    @_guard
    def worker_open_shplonk_finish(self, handles: Sequence[int], h_handle: int, points: Sequence[str],
                                   opened: Sequence[Sequence[int]], coeffs: Sequence[str], u: str):
        """Extension: round B of a SHPLONK opening: the value v and the proof pi of the combination of the rows and h (the
        set worker_commit_shplonk made) at u.  u must be drawn after W and differ from every point.  The proof is (W, pi)."""
        hs, hh = _handles(handles), _handles([h_handle])[0]
        a, c = self._shplonk_args("worker_open_shplonk_finish", points, opened, coeffs)
        ub = codec.fr_to_be32(u)
        if ub in a:
            raise codec.CodecError("worker_open_shplonk_finish: u must not be one of the points")
        v, pf = self.engine.open_shplonk_finish(hs, hh, a, opened, c, ub)
        return {"value": codec.be32_to_fr(v), "proof": codec.g1_to_b64(pf)}

    @_guard
    def worker_commit_grand_product(self, wire_handles: Sequence[int], sigma_handles: Sequence[int], shifts: Sequence[str],
                                    beta: str, gamma: str):
        """Extension: the permutation grand product z over the rows of committed sets (wire rows a_j from wire_handles,
        permutation rows sigma_j from sigma_handles, one shift per row), computed and committed on the device as a new
        one-row set.  Returns its handle, its commitment and the closing value (1 when the permutation holds).  beta and
        gamma must be drawn after the wire commitments are fixed."""
        hw, hs, sh, ch = self._grand_product_args("worker_commit_grand_product", wire_handles, sigma_handles, shifts,
                                                  (beta, gamma), "beta and gamma")
        return self._with_closing(*self.engine.commit_grand_product(hw, hs, sh, *ch))

    # ---- one parser per builder behind its plain, _zk, _sel and _chain forms: `what` is the public method's name
    @staticmethod
    def _grand_product_args(what: str, wire_handles, sigma_handles, shifts, challenges, names: str) -> tuple:
        """(wire handles, sigma handles, the shifts' bytes, the challenges' bytes); `names` words the challenges"""
        hw, hs = _handles(wire_handles), _handles(sigma_handles)
        if not 1 <= len(shifts) <= KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"{what}: {len(shifts)} shifts, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        sc = [codec.fr_to_be32(x) for x in list(shifts) + list(challenges)]
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in sc):
            raise codec.CodecError(f"{what}: shifts, {names} must be canonical scalars (< r)")
        return hw, hs, sc[:len(shifts)], sc[len(shifts):]

    @staticmethod
    def _lookup_shape(what: str, n_lookups, width) -> tuple:
        try:
            n_lookups, width = int(n_lookups), int(width)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: n_lookups and width must be integers: {e!r}") from e
        if n_lookups < 1 or width < 1 or n_lookups * width > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"{what}: n_lookups = {n_lookups}, width = {width}, expected both >= 1 "
                                   f"and n_lookups * width <= {KZG_MAX_BATCH_OPEN}")
        return n_lookups, width

    def _lookup_sum_args(self, what: str, input_handles, table_handles, mult_handle, n_lookups, width, theta, beta,
                         sel=None) -> tuple:
        """The engine's arguments up to beta; sel = (sel_handles, sel_index) puts the selectors behind the handles (_sel)"""
        hi, ht, hm = _handles(input_handles), _handles(table_handles), _handles([mult_handle])[0]
        n_lookups, width = self._lookup_shape(what, n_lookups, width)
        sel = self._selectors(what, *sel, n_lookups) if sel else ()
        sc = [codec.fr_to_be32(x) for x in (theta, beta)]
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in sc):
            raise codec.CodecError(f"{what}: theta and beta must be canonical scalars (< r)")
        return (hi, ht, hm, *sel, n_lookups, width, sc[0], sc[1])

    def _multiplicities_args(self, what: str, input_handles, table_handles, n_lookups, width, sel=None) -> tuple:
        """The engine's arguments up to width; sel as for _lookup_sum_args"""
        hi, ht = _handles(input_handles), _handles(table_handles)
        n_lookups, width = self._lookup_shape(what, n_lookups, width)
        return (hi, ht, *(self._selectors(what, *sel, n_lookups) if sel else ()), n_lookups, width)

    @staticmethod
    def _with_closing(rs, closing) -> dict:
        return {"handle": int(rs.handle), "commitment": codec.g1_to_b64(rs.commitments[0]),
                "closing": codec.be32_to_fr(closing)}

    @staticmethod
    def _with_missing(rs, missing) -> dict:
        return {"handle": int(rs.handle), "commitment": codec.g1_to_b64(rs.commitments[0]), "missing": int(missing)}

    @_guard
    def worker_commit_lookup_sum(self, input_handles: Sequence[int], table_handles: Sequence[int], mult_handle: int,
                                 n_lookups: int, width: int, theta: str, beta: str):
        """Extension: the running sum S of a log-derivative lookup argument over the rows of committed sets (n_lookups *
        width input rows from input_handles, lookup-major; width table columns from table_handles; the multiplicities in
        the one-row set mult_handle), computed and committed on the device as a new one-row set.  Returns its handle, its
        commitment and the closing value (0 when the sum closes).  theta and beta must be drawn after the commitments of
        the inputs, the table and the multiplicities are fixed."""
        args = self._lookup_sum_args("worker_commit_lookup_sum", input_handles, table_handles, mult_handle, n_lookups, width,
                                     theta, beta)
        return self._with_closing(*self.engine.commit_lookup_sum(*args))

    @_guard
    def worker_commit_multiplicities(self, input_handles: Sequence[int], table_handles: Sequence[int], n_lookups: int,
                                     width: int):
        """Extension: the multiplicity row m of a lookup argument over the rows of committed sets (n_lookups * width input
        rows from input_handles, lookup-major; width table columns from table_handles), joined and committed on the device
        as a new one-row set.  Returns its handle, its commitment and `missing`, the number of looked-up cells whose tuple is
        no row of the table (0 when every lookup is satisfied).  The handle goes straight into worker_commit_lookup_sum as
        mult_handle; theta and beta are drawn after this commitment."""
        args = self._multiplicities_args("worker_commit_multiplicities", input_handles, table_handles, n_lookups, width)
        return self._with_missing(*self.engine.commit_multiplicities(*args))

    @_guard
    def worker_commit_quotient(self, handles: Sequence[int], terms, perm=None, ext_log: int = 2, n_pieces: int = 3):
        """Extension: the PLONK quotient t over the rows of committed sets, computed and committed on the device as a new set
        of n_pieces rows.  terms: [coefficient, [row indices]] per gate term; perm: None or {"wires", "sigmas", "z",
        "shifts", "beta", "gamma", "alpha"} (row indices and scalars).  Returns the new handle and the pieces' commitments.
        alpha must be drawn after z's commitment is fixed, beta and gamma after the wires."""
        hs = _handles(handles)
        try:
            ext_log, n_pieces = int(ext_log), int(n_pieces)
            tt = [(codec.fr_to_be32(c), [int(j) for j in rows]) for c, rows in terms]
            pp = None
            if perm is not None and len(perm["wires"]):   # (no wire: the part is off, as perm->k == 0 in C)
                pp = {"wires": [int(j) for j in perm["wires"]], "sigmas": [int(j) for j in perm["sigmas"]], "z": int(perm["z"]),
                      "shifts": [codec.fr_to_be32(x) for x in perm["shifts"]], "beta": codec.fr_to_be32(perm["beta"]),
                      "gamma": codec.fr_to_be32(perm["gamma"]), "alpha": codec.fr_to_be32(perm["alpha"])}
        except (TypeError, ValueError, KeyError) as e:
            raise codec.CodecError(f"worker_commit_quotient: malformed terms or permutation part: {e!r}") from e
        scal = [c for c, _ in tt] + (pp["shifts"] + [pp["beta"], pp["gamma"], pp["alpha"]] if pp else [])
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in scal):
            raise codec.CodecError("worker_commit_quotient: coefficients, shifts and challenges must be canonical scalars (< r)")
        rs = self.engine.commit_quotient(hs, tt, pp, ext_log, n_pieces)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @_guard
    def worker_commit_quotient_ext(self, handles: Sequence[int], terms, perm=None, lookup=None, ext_log: int = 2,
                                   n_pieces: int = 3):
        """Extension: worker_commit_quotient with rotated gate factors and the lookup (logUp) relation.  terms:
        [coefficient, [factors]] per gate term, a factor being a row index or a [row, rot] pair (the row at t + rot on the
        domain); perm as in worker_commit_quotient; lookup: None or {"inputs", "table", "mult", "sum", "width", "theta",
        "beta", "alpha"} (row indices, the tuple width and scalars; theta and beta those of worker_commit_lookup_sum).
        Returns the new handle and the pieces' commitments.  alpha must be drawn after the commitments of S and z are fixed."""
        hs = _handles(handles)
        try:
            ext_log, n_pieces = int(ext_log), int(n_pieces)
            tt = [(codec.fr_to_be32(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in fs])
                  for c, fs in terms]
            if any(isinstance(f, (tuple, list)) and len(f) != 2 for _, fs in terms for f in fs):
                raise ValueError("a factor is a row index or a [row, rot] pair")
            pp = None
            if perm is not None and len(perm["wires"]):   # (no wire: the part is off, as perm->k == 0 in C)
                pp = {"wires": [int(j) for j in perm["wires"]], "sigmas": [int(j) for j in perm["sigmas"]], "z": int(perm["z"]),
                      "shifts": [codec.fr_to_be32(x) for x in perm["shifts"]], "beta": codec.fr_to_be32(perm["beta"]),
                      "gamma": codec.fr_to_be32(perm["gamma"]), "alpha": codec.fr_to_be32(perm["alpha"])}
            ll = None
            if lookup is not None:
                ll = {"inputs": [int(j) for j in lookup["inputs"]], "table": [int(j) for j in lookup["table"]],
                      "mult": int(lookup["mult"]), "sum": int(lookup["sum"]), "width": int(lookup["width"]),
                      "theta": codec.fr_to_be32(lookup["theta"]), "beta": codec.fr_to_be32(lookup["beta"]),
                      "alpha": codec.fr_to_be32(lookup["alpha"])}
        except (TypeError, ValueError, KeyError, IndexError) as e:
            raise codec.CodecError(f"worker_commit_quotient_ext: malformed terms, permutation or lookup part: {e!r}") from e
        scal = [c for c, _ in tt] + (pp["shifts"] + [pp["beta"], pp["gamma"], pp["alpha"]] if pp else []) + \
            ([ll["theta"], ll["beta"], ll["alpha"]] if ll else [])
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in scal):
            raise codec.CodecError("worker_commit_quotient_ext: coefficients, shifts and challenges must be canonical scalars "
                                   "(< r)")
        rs = self.engine.commit_quotient_ext(hs, tt, pp, ll, ext_log, n_pieces)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    # ---- the builders with blinding rows (kzg_rows_commit_*_zk): rows [0, usable) carry the circuit, row `usable` closes the
    # running value and rows usable + 1 .. T - 1 take `tail`, the caller's fresh random scalars (T - usable - 1 of them)
    @staticmethod
    def _blind(what: str, usable, tail) -> tuple:
        try:
            usable = int(usable)
            tb = [codec.fr_to_be32(x) for x in (tail or [])]
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: usable must be an integer and the tail a list of scalars: {e!r}") from e
        if usable < 0 or any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in tb):
            raise codec.CodecError(f"{what}: usable must not be negative and the tail scalars must be canonical (< r)")
        return usable, tb

    @classmethod
    def _layout(cls, what: str, usable, tail, null_means: str = "all rows are read") -> tuple:
        """usable and tail as the column builders take them: (None, []) for usable = null, which takes no tail"""
        if usable is None:
            if tail:
                raise codec.CodecError(f"{what}: a tail needs usable (null: {null_means})")
            return None, []
        usable, tb = cls._blind(what, usable, tail)
        if usable == 0:
            raise codec.CodecError(f"{what}: usable must be in [1, T - 1] (null: {null_means})")
        return usable, tb

    @staticmethod
    def _unit_objects(what: str, units, slot_lists=(), slots=(), params=_NO_PARAMS) -> list:
        """The units of a unit builder's request as the engine's encoder takes them: every unit an object; the entries of the
        fields slot_lists and the fields slots themselves become tuples where they are lists (["imm", value]).  params: the
        object that leads the request, where the builder has one in this check"""
        with_params = params is not _NO_PARAMS
        head = "params must be an object and units a list of objects" if with_params else "units must be a list of objects"
        try:
            if with_params and not isinstance(params, dict):
                raise ValueError(f"params is an object: {params!r}")
            recs = []
            for un in units:
                if not isinstance(un, dict):
                    raise ValueError(f"a unit is an object: {un!r}")
                rec = dict(un)
                for name in slot_lists:
                    if isinstance(rec.get(name), (list, tuple)):
                        rec[name] = [tuple(v) if isinstance(v, (list, tuple)) else v for v in rec[name]]
                for name in slots:
                    if isinstance(rec.get(name), (list, tuple)):
                        rec[name] = tuple(rec[name])
                recs.append(rec)
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: {head}: {e!r}") from e
        if not recs:
            raise codec.CodecError(f"{what}: units must not be empty")
        return recs

    @_guard
    def worker_commit_grand_product_zk(self, wire_handles: Sequence[int], sigma_handles: Sequence[int], shifts: Sequence[str],
                                       beta: str, gamma: str, usable: int, tail: Sequence[str]):
        """Extension: worker_commit_grand_product over the first `usable` rows only: z(w^usable) is the closing value (1 when
        the permutation holds on the usable rows) and z's rows behind it are `tail`.  Rows >= usable of the wires and sigmas
        do not enter the product.  The library draws no randomness: the tail must be fresh per proof."""
        hw, hs, sh, ch = self._grand_product_args("worker_commit_grand_product_zk", wire_handles, sigma_handles, shifts,
                                                  (beta, gamma), "beta and gamma")
        usable, tb = self._blind("worker_commit_grand_product_zk", usable, tail)
        return self._with_closing(*self.engine.commit_grand_product_zk(hw, hs, sh, *ch, usable, tb))

    @_guard
    def worker_commit_lookup_sum_zk(self, input_handles: Sequence[int], table_handles: Sequence[int], mult_handle: int,
                                    n_lookups: int, width: int, theta: str, beta: str, usable: int, tail: Sequence[str]):
        """Extension: worker_commit_lookup_sum over the first `usable` rows only: S(w^usable) is the closing value (0 when
        the sum closes on the usable rows) and S's rows behind it are `tail`."""
        args = self._lookup_sum_args("worker_commit_lookup_sum_zk", input_handles, table_handles, mult_handle, n_lookups, width,
                                     theta, beta)
        usable, tb = self._blind("worker_commit_lookup_sum_zk", usable, tail)
        return self._with_closing(*self.engine.commit_lookup_sum_zk(*args, usable, tb))

    @_guard
    def worker_commit_multiplicities_zk(self, input_handles: Sequence[int], table_handles: Sequence[int], n_lookups: int,
                                        width: int, usable: int, tail: Sequence[str]):
        """Extension: worker_commit_multiplicities over the first `usable` table rows and input cells only (`missing` counts
        those cells alone): m(w^usable) = 0 and m's rows behind it are `tail`."""
        args = self._multiplicities_args("worker_commit_multiplicities_zk", input_handles, table_handles, n_lookups, width)
        usable, tb = self._blind("worker_commit_multiplicities_zk", usable, tail)
        return self._with_missing(*self.engine.commit_multiplicities_zk(*args, usable, tb))

    # ---- the two lookup builders with per-row selectors (kzg_rows_commit_*_sel)
    @staticmethod
    def _selectors(what: str, sel_handles, sel_index, n_lookups: int) -> tuple:
        """sel_handles: [] or row-set handles; sel_index: per lookup None (no selector) or a row of their concatenation"""
        hs = _handles(sel_handles) if sel_handles else []
        try:
            idx = [None if j is None else int(j) for j in sel_index]
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: sel_index must be a list of row indices or nulls: {e!r}") from e
        if len(idx) != n_lookups or any(j is not None and not 0 <= j < KZG_MAX_BATCH_OPEN for j in idx):
            raise codec.CodecError(f"{what}: sel_index must hold n_lookups = {n_lookups} entries, each null or a row index below "
                                   f"{KZG_MAX_BATCH_OPEN}")
        if not hs and any(j is not None for j in idx):
            raise codec.CodecError(f"{what}: sel_index names a row but no selector handle was given")
        return hs, idx

    @_guard
    def worker_commit_lookup_sum_sel(self, input_handles: Sequence[int], table_handles: Sequence[int], mult_handle: int,
                                     sel_handles: Sequence[int], sel_index: Sequence[Optional[int]], n_lookups: int, width: int,
                                     theta: str, beta: str, usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: worker_commit_lookup_sum (usable = None) or worker_commit_lookup_sum_zk with per-row selectors: the
        fraction of lookup l has the numerator q_l, row sel_index[l] of the concatenated rows of the sel_handles sets (null: the
        constant 1).  The sum closes against worker_commit_multiplicities_sel's m when q_l is 0 or 1 on the rows that count."""
        args = self._lookup_sum_args("worker_commit_lookup_sum_sel", input_handles, table_handles, mult_handle, n_lookups, width,
                                     theta, beta, (sel_handles, sel_index))
        usable, tb = (None, []) if usable is None else self._blind("worker_commit_lookup_sum_sel", usable, tail)
        return self._with_closing(*self.engine.commit_lookup_sum_sel(*args, usable, tb))

    @_guard
    def worker_commit_multiplicities_sel(self, input_handles: Sequence[int], table_handles: Sequence[int],
                                         sel_handles: Sequence[int], sel_index: Sequence[Optional[int]], n_lookups: int,
                                         width: int, usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: worker_commit_multiplicities (usable = None) or worker_commit_multiplicities_zk with per-row selectors:
        cell (l, t) is probed, and can be `missing`, only where row sel_index[l] of the concatenated rows of the sel_handles
        sets is not zero at t (null: every cell).  A disabled cell may hold anything."""
        args = self._multiplicities_args("worker_commit_multiplicities_sel", input_handles, table_handles, n_lookups, width,
                                         (sel_handles, sel_index))
        usable, tb = (None, []) if usable is None else self._blind("worker_commit_multiplicities_sel", usable, tail)
        return self._with_missing(*self.engine.commit_multiplicities_sel(*args, usable, tb))

    # ---- the shuffle: ONE call for its plain, selector and blinding-rows forms
    def _shuffle_args(self, what: str, input_handles, shuffle_handles, n_groups, width, theta, gamma, sel_handles, input_sel,
                      shuffle_sel, usable, tail) -> tuple:
        """The engine's arguments, in its order"""
        hi, hs = _handles(input_handles), _handles(shuffle_handles)
        n_groups, width = self._lookup_shape(what, n_groups, width)
        hq, sides = _handles(sel_handles) if sel_handles else [], []
        for idx in (input_sel, shuffle_sel):
            sides.append(None if idx is None else self._selectors(what, hq, idx, n_groups)[1])
        sc = [codec.fr_to_be32(x) for x in (theta, gamma)]
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in sc):
            raise codec.CodecError(f"{what}: theta and gamma must be canonical scalars (< r)")
        usable, tb = (None, []) if usable is None else self._blind(what, usable, tail)
        return (hi, hs, n_groups, width, sc[0], sc[1], hq, sides[0], sides[1], usable, tb)

    @_guard
    def worker_commit_shuffle(self, input_handles: Sequence[int], shuffle_handles: Sequence[int], n_groups: int, width: int,
                              theta: str, gamma: str, sel_handles: Optional[Sequence[int]] = None,
                              input_sel: Optional[Sequence[Optional[int]]] = None,
                              shuffle_sel: Optional[Sequence[Optional[int]]] = None, usable: Optional[int] = None,
                              tail: Sequence[str] = ()):
        """Extension: the running product z of a shuffle argument over the rows of committed sets (n_groups * width input
        rows from input_handles, group-major, against as many shuffle rows from shuffle_handles), computed and committed on
        the device as a new one-row set.  input_sel / shuffle_sel: null, or per group null or that side's selector row in the
        concatenated rows of the sel_handles sets (a disabled cell contributes the factor 1).  usable = null is the plain
        layout; otherwise z(w^usable) is the closing value and z's rows behind it are `tail`, as for
        worker_commit_grand_product_zk.  Returns its handle, its commitment and the closing value (1 when the product
        closes).  theta and gamma must be drawn after the commitments of all input and shuffle rows are fixed; the argument is
        the relation of shuffle_quotient_terms in the caller's quotient, not the closing value."""
        args = self._shuffle_args("worker_commit_shuffle", input_handles, shuffle_handles, n_groups, width, theta, gamma,
                                  sel_handles, input_sel, shuffle_sel, usable, tail)
        return self._with_closing(*self.engine.commit_shuffle(*args))

    # ---- the sorted side of a shuffle: the columns of committed sets, sorted as tuples on the device
    @_guard
    def worker_commit_sorted(self, input_handles: Sequence[int], width: int, n_keys: Optional[int] = None,
                             usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: the `width` rows of the input_handles sets, read as the columns of one tuple per row, stably sorted on the
        device and committed as a new set of `width` rows: ascending by the canonical integers of the first n_keys columns
        (null: all), column 0 most significant, ties by source row; the other columns travel as payload.  usable = null sorts
        all T rows; otherwise only rows [0, usable) are sorted (the source rows behind are not read) and row usable + s of
        column c is tail[c * (T - usable) + s] -- there is no closing row.  Returns the handle and the `width` commitments.
        Nothing here is a proof: the argument is worker_commit_shuffle over the inputs and this set plus the caller's
        adjacent-row gate, with theta and gamma drawn after these commitments are fixed."""
        what = "worker_commit_sorted"
        hs = _handles(input_handles)
        try:
            width = int(width)
            n_keys = width if n_keys is None else int(n_keys)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: width and n_keys must be integers: {e!r}") from e
        if not 1 <= width <= KZG_MAX_BATCH_OPEN or not 1 <= n_keys <= width:
            raise codec.CodecError(f"{what}: width must be in [1, {KZG_MAX_BATCH_OPEN}] and n_keys in [1, width]")
        usable, tb = self._layout(what, usable, tail, "all rows are sorted")
        rs = self.engine.commit_sorted(hs, width, n_keys, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    # ---- the helper columns of zero tests and range checks: functions of one resident column, built on the device
    @_guard
    def worker_commit_derived(self, input_handles: Sequence[int], ops: Sequence[Sequence], usable: Optional[int] = None,
                              tail: Sequence[str] = ()):
        """Extension: helper columns of the rows of the input_handles sets, computed and committed on the device as one new set.
        ops: ["inv0", row] gives the row 1 / x with 0 where x = 0 (the IsZero gadget), ["inv0", row, true] also the bit row
        behind it (1 where x = 0); ["limbs", row, bits, count] the `count` limbs of `bits` bits of x's canonical integer, least
        significant first (range checks: the limbs go into worker_commit_multiplicities against a 2^bits table).  usable = null
        reads all T rows; otherwise only rows [0, usable) are read and row usable + s of output column c is
        tail[c * (T - usable) + s] -- there is no closing row.  Returns the handle, the commitments of all output rows in the
        order of ops, and one count per op: the zero cells of an inv0 op, the cells at or above 2^(bits * count) of a limbs op
        (0 when the range check can hold).  Nothing here is a proof: the argument is the caller's gates and lookups over these
        rows, with every challenge drawn after these commitments are fixed."""
        what = "worker_commit_derived"
        hs = _handles(input_handles)
        try:
            recs = []
            for op in ops:
                name = op[0]
                if name == "inv0" and len(op) in (2, 3):
                    recs.append(("inv0", int(op[1]), bool(op[2])) if len(op) == 3 else ("inv0", int(op[1])))
                elif name == "limbs" and len(op) == 4:
                    recs.append(("limbs", int(op[1]), int(op[2]), int(op[3])))
                else:
                    raise ValueError(f"unknown op {op!r}")
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f'{what}: ops must be a list of ["inv0", row], ["inv0", row, with_bit] or '
                                   f'["limbs", row, bits, count]: {e!r}') from e
        if not recs:
            raise codec.CodecError(f"{what}: ops must not be empty")
        usable, tb = self._layout(what, usable, tail)
        rs, counts = self.engine.commit_derived(hs, recs, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "counts": [int(v) for v in counts]}

    # ---- columns that are plain arithmetic in resident columns, and gates checked row by row, on the device
    @_guard
    def worker_commit_expr(self, input_handles: Sequence[int], exprs: Sequence[Sequence], usable: Optional[int] = None,
                           tail: Sequence[str] = ()):
        """Extension: expression columns over the rows of the input_handles sets, evaluated on the device: v[t] = sum_u c_u
        prod_f row[(t + rot) mod T].  exprs: a list whose entries are [terms] (the column is committed) or [terms, true] (a
        check: evaluated and counted only); terms as in worker_commit_quotient_ext: [coefficient, [factors]] per term, a factor
        a row index or a [row, rot] pair, at most 8 factors per term and 16 terms.  The committed expressions become, in their
        order, the rows of ONE new set.  usable = null evaluates all T rows; otherwise only rows [0, usable) and row usable + s
        of committed column c is tail[c * (T - usable) + s] -- there is no closing row.  Returns the handle (null when every
        entry is a check), the commitments, and per entry `nonzero`, the number of non-zero cells among the rows evaluated,
        and `first`, the smallest such row (null: none).  Nothing here is a proof: a committed column is prover data and the
        argument is the caller's gate in the quotient; a zero count only tells the prover that the gate holds."""
        what = "worker_commit_expr"
        hs = _handles(input_handles)
        try:
            recs = []
            for ent in exprs:
                if isinstance(ent, (str, bytes)) or len(ent) not in (1, 2) or (len(ent) == 2 and not isinstance(ent[1], bool)):
                    raise ValueError(f"an entry is [terms] or [terms, check]: {ent!r}")
                if any(isinstance(f, (tuple, list)) and len(f) != 2 for _, fs in ent[0] for f in fs):
                    raise ValueError("a factor is a row index or a [row, rot] pair")
                tt = [(codec.fr_to_be32(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in fs])
                      for c, fs in ent[0]]
                recs.append((tt, len(ent) == 2 and ent[1]))
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: exprs must be a list of [terms] or [terms, check] with terms a list of "
                                   f"[coefficient, [factors]]: {e!r}") from e
        if not recs:
            raise codec.CodecError(f"{what}: exprs must not be empty")
        if any(int.from_bytes(c, "big") >= codec.R_MODULUS for tt, _ in recs for c, _ in tt):
            raise codec.CodecError(f"{what}: coefficients must be canonical scalars (< r)")
        usable, tb = self._layout(what, usable, tail, "all rows are evaluated")
        rs, nonzero, first = self.engine.commit_expr(hs, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments],
                "nonzero": nonzero, "first": first}

    # ---- running values along the rows, v[t + 1] = A[t] v[t] + B[t] with A and B expressions in resident columns, on the device
    @_guard
    def worker_commit_recurrence(self, input_handles: Sequence[int], recs: Sequence[Sequence], usable: Optional[int] = None,
                                 tail: Sequence[str] = ()):
        """Extension: first-order recurrence columns over the rows of the input_handles sets, built on the device: v[0] = start,
        v[t + 1] = A[t] v[t] + B[t].  recs: a list of [mul_terms, add_terms, start] entries; both term lists as in
        worker_commit_expr ([coefficient, [factors]] per term, a factor a row index or a [row, rot] pair, at most 8 factors per
        term and 16 terms); an empty mul_terms is A = 1, an empty add_terms is B = 0, both empty is refused.  A zero multiplier
        restarts the value at the addend.  The recurrences become, in their order, the rows of ONE new set.  usable = null: rows
        0 .. T - 1 hold v[0] .. v[T - 1] and `closings` holds v[T], which equals start exactly when the relation holds cyclically;
        otherwise rows 0 .. usable hold v[0] .. v[usable], the last of them the closing value, and row usable + 1 + s of column c
        is tail[c * (T - usable - 1) + s].  Returns the handle, the commitments and the closings.  Nothing here is a proof: the
        column is prover data and the argument is the caller's gate v(wX) - A v - B in the quotient plus the boundary gate."""
        what = "worker_commit_recurrence"
        hs = _handles(input_handles)

        def side(terms):
            if any(isinstance(f, (tuple, list)) and len(f) != 2 for _, fs in terms for f in fs):
                raise ValueError("a factor is a row index or a [row, rot] pair")
            return [(codec.fr_to_be32(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in fs])
                    for c, fs in terms]
        try:
            rr = []
            for ent in recs:
                if isinstance(ent, (str, bytes)) or len(ent) != 3:
                    raise ValueError(f"an entry is [mul_terms, add_terms, start]: {ent!r}")
                rr.append((side(ent[0]), side(ent[1]), codec.fr_to_be32(ent[2])))
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: recs must be a list of [mul_terms, add_terms, start] with terms a list of "
                                   f"[coefficient, [factors]]: {e!r}") from e
        if not rr:
            raise codec.CodecError(f"{what}: recs must not be empty")
        if any(not m and not a for m, a, _ in rr):
            raise codec.CodecError(f"{what}: mul_terms and add_terms must not both be empty")
        if any(int.from_bytes(c, "big") >= codec.R_MODULUS for m, a, _ in rr for c, _ in m + a) or any(
                int.from_bytes(st, "big") >= codec.R_MODULUS for _, _, st in rr):
            raise codec.CodecError(f"{what}: coefficients and starts must be canonical scalars (< r)")
        usable, tb = self._layout(what, usable, tail, "the plain layout")
        rs, closings = self.engine.commit_recurrence(hs, rr, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "closings": [codec.be32_to_fr(c) for c in closings]}

    # ---- columns read out of a resident table, by key or by row index, on the device
    @_guard
    def worker_commit_fetch(self, input_handles: Sequence[int], table_handles: Sequence[int], n_reads: int, n_keys: int,
                            with_index: bool = False, usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: columns fetched from a table that is already resident.  The rows of the table_handles sets are the
        table's columns, the first n_keys the key and the others the payload; the rows of the input_handles sets are n_reads
        reads of n_keys rows each (read-major).  Every cell takes the payload of the SMALLEST table row whose key equals the
        cell's key in all n_keys columns (with_index: that row number leads the read's columns), or zeros where there is
        none: c = a XOR b from the table (a, b, a ^ b), a ROM read, the value of a sorted memory back in program order.  With
        n_keys = 0 a read is ONE row of row indices, every table column is payload and an index at or beyond the table's
        rows is a miss.  All outputs form ONE new set in read order.  usable = null reads all T rows; otherwise only cells and
        table rows [0, usable) take part and row usable + s of output column c is tail[c * (T - usable) + s] -- there is no
        closing row.  Returns the handle, the commitments, and per read `missing`, the number of cells without a table row,
        and `first_missing`, the smallest such cell (null: none).  A miss is no error.  Nothing here is a proof: the fetched
        rows are prover data and the argument is the lookup of (key, payload) in the table."""
        what = "worker_commit_fetch"
        hi, ht = _handles(input_handles), _handles(table_handles)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (n_reads, n_keys)) or not isinstance(with_index, bool):
            raise codec.CodecError(f"{what}: n_reads and n_keys must be integers and with_index a boolean")
        if n_reads < 1 or n_keys < 0 or n_reads * max(n_keys, 1) > KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"{what}: n_reads >= 1, n_keys >= 0 and n_reads * max(n_keys, 1) <= {KZG_MAX_BATCH_OPEN}")
        if with_index and n_keys == 0:
            raise codec.CodecError(f"{what}: with_index needs n_keys >= 1 (by row index the input row is the index)")
        usable, tb = self._layout(what, usable, tail)
        rs, missing, first = self.engine.commit_fetch(hi, ht, n_reads, n_keys, with_index, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "missing": [int(v) for v in missing], "first_missing": first}

    # ---- the permutation's sigma columns from variable labels, and the copy check over the same labels
    @staticmethod
    def _sigma_args(what: str, usable, free_label) -> tuple:
        """(usable or None, the free label's bytes or None)"""
        if usable is not None:
            if isinstance(usable, bool) or not isinstance(usable, int) or usable < 1:
                raise codec.CodecError(f"{what}: usable must be an integer in [1, T - 1] (null: all rows take part)")
        fl = None
        if free_label is not None:
            fl = codec.fr_to_be32(free_label)
            if int.from_bytes(fl, "big") >= codec.R_MODULUS:
                raise codec.CodecError(f"{what}: the free label must be a canonical scalar (< r)")
        return usable, fl

    @_guard
    def worker_commit_sigma(self, label_handles: Sequence[int], shifts: Sequence[str], usable: Optional[int] = None,
                            free_label: Optional[str] = None):
        """Extension: the permutation rows sigma_0 .. sigma_{k-1} that worker_commit_grand_product takes, built on the device
        from variable labels.  The rows of the label_handles sets are k = len(shifts) label columns (commit them with
        worker_commit_rows_typed); cells with equal labels are one copy class, and sigma runs through every class as one
        cycle in ascending flat index column * T + row.  usable = null: all T rows take part; otherwise rows [0, usable) do
        and the rows behind map to themselves.  A cell whose label is free_label (null: no such label) maps to itself.
        Returns the handle, the k commitments, `classes` (distinct non-free labels among the participating cells) and `fixed`
        (participating cells that map to themselves).  sigma is a fixed column of the circuit, no proof of anything."""
        what = "worker_commit_sigma"
        hl = _handles(label_handles)
        if not 1 <= len(shifts) <= KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"{what}: {len(shifts)} shifts, expected 1 .. {KZG_MAX_BATCH_OPEN}")
        sh = [codec.fr_to_be32(x) for x in shifts]
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in sh):
            raise codec.CodecError(f"{what}: the shifts must be canonical scalars (< r)")
        usable, fl = self._sigma_args(what, usable, free_label)
        commitments, rs, stats = self.engine.commit_sigma(hl, sh, usable, fl)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in commitments],
                "classes": int(stats["classes"]), "fixed": int(stats["fixed"])}

    @_guard
    def worker_check_copies(self, wire_handles: Sequence[int], label_handles: Sequence[int], usable: Optional[int] = None,
                            free_label: Optional[str] = None):
        """Extension: the copy constraints of worker_commit_sigma's labels checked against the wire columns, cell by cell on
        the device.  A participating, non-free cell is a violation when its value differs from that of its class's smallest
        cell.  Returns `violations` and `first`, the [column, row] of the smallest violating flat index (null: none).  No set
        is created and no MSM runs.  A count convinces no verifier: the argument is the grand product over sigma."""
        what = "worker_check_copies"
        hw, hl = _handles(wire_handles), _handles(label_handles)
        usable, fl = self._sigma_args(what, usable, free_label)
        res = self.engine.check_copies(hw, hl, usable, fl)
        return {"violations": int(res["violations"]), "first": None if res["first"] is None else [int(v) for v in res["first"]]}

    # ---- machine-word arithmetic on resident columns: bitwise ops, carries, high products, quotients, shifts, on the device
    @_guard
    def worker_commit_int(self, input_handles: Sequence[int], ops: Sequence[Sequence], usable: Optional[int] = None,
                          tail: Sequence[str] = ()):
        """Extension: integer ALU columns of the rows of the input_handles sets, computed and committed on the device as one new
        set.  ops: [kind, w, a, b] or [kind, w, a, b, count] with kind one of "and" "or" "xor" "add" "sub" "mul" "divmod"
        "split", w the width in [1, 64], a a row, b a row or ["imm", value], count 1 or 2.  The operands are the cells'
        canonical integers reduced to their low w bits; the rows of an op, in this order: a op b; the sum and its carry; the
        difference and its borrow (1 where a < b); the low and the high word of the product; the quotient and the remainder
        (2^w - 1 and a where b = 0); a >> s and a mod 2^s with the shift s as second operand.  usable = null reads all T rows;
        otherwise only rows [0, usable) are read and row usable + s of output column c is tail[c * (T - usable) + s] -- there is
        no closing row.  Returns the handle, the commitments of all output rows in the order of ops, and per op `counts`, the
        cells read with an operand at or above 2^w (a shift cell: above w), and `first`, the smallest such row (null: none).
        Nothing here is a proof: the rows are prover data and the argument is the caller's gates and range lookups over them."""
        what = "worker_commit_int"
        hs = _handles(input_handles)
        try:
            recs = []
            for op in ops:
                if isinstance(op, (str, bytes)) or len(op) not in (4, 5):
                    raise ValueError(f"an op is [kind, w, a, b] or [kind, w, a, b, count]: {op!r}")
                b = op[3]
                if isinstance(b, (list, tuple)):
                    if len(b) != 2 or b[0] != "imm":
                        raise ValueError(f'an immediate is ["imm", value]: {b!r}')
                    b = ("imm", int(b[1]))
                else:
                    b = int(b)
                recs.append((str(op[0]), int(op[1]), int(op[2]), b) + ((int(op[4]),) if len(op) == 5 else ()))
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: ops must be a list of [kind, w, a, b] or [kind, w, a, b, count]: {e!r}") from e
        if not recs:
            raise codec.CodecError(f"{what}: ops must not be empty")
        usable, tb = self._layout(what, usable, tail)
        rs, counts, first = self.engine.commit_int(hs, recs, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "counts": counts, "first": first}

    # ---- the same arithmetic and its signed kinds with the kind chosen per row: the ALU column of a CPU table
    @_guard
    def worker_commit_alu(self, input_handles: Sequence[int], program: Sequence, units: Sequence[Sequence],
                          usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: ALU columns whose KIND an op-code column picks per row, computed and committed on the device as one new
        set.  program: at most 64 entries, the index the op-code, each null (idle), [kind, w] or [kind, w, ["imm", value]]
        with kind one of "and" "or" "xor" "add" "sub" "mul" "divmod" "split" "ltu" "lt" "eq" "sll" "srl" "sra" "rotl" "rotr"
        "mulhu" "mulh" "mulhsu" "div" "rem" "remu" "sext" and w the width in [1, 64].  units: 1 to 8 entries [op_row, a, b] or
        [op_row, a, b, count], rows of the concatenated input sets, count 1 or 2, at most 16 output rows in all.  Per cell, c is
        the integer of op_row: c beyond the program gives 0 and is counted as unknown; a null entry gives 0 and reads nothing;
        otherwise the entry's kind acts on a and b (or the entry's immediate, and then b is neither read nor counted) reduced to
        their low w bits, as in worker_commit_int, and writes row 0 and row 1 of that kind (include/kzg_mi355x.h lists them).
        usable and tail: as for worker_commit_int.  Returns the handle, the commitments of all output rows unit by unit, and
        per unit `counts` (cells read with an operand out of range), `first` (the smallest such row, null: none), `unknown`
        and `first_unknown` (the same for unknown op-codes).  Nothing here is a proof: the rows are prover data."""
        what = "worker_commit_alu"
        hs = _handles(input_handles)
        try:
            prog = []
            for en in program:
                if en is None:
                    prog.append(None)
                    continue
                if isinstance(en, (str, bytes)) or len(en) not in (2, 3):
                    raise ValueError(f'an entry is null, [kind, w] or [kind, w, ["imm", value]]: {en!r}')
                rec = (str(en[0]), int(en[1]))
                if len(en) == 3:
                    imm = en[2]
                    if not isinstance(imm, (list, tuple)) or len(imm) != 2 or imm[0] != "imm":
                        raise ValueError(f'an immediate is ["imm", value]: {imm!r}')
                    rec += (("imm", int(imm[1])),)
                prog.append(rec)
            us = []
            for un in units:
                if isinstance(un, (str, bytes)) or len(un) not in (3, 4):
                    raise ValueError(f"a unit is [op_row, a, b] or [op_row, a, b, count]: {un!r}")
                us.append(tuple(int(v) for v in un))
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: program must be a list of null, [kind, w] or [kind, w, [\"imm\", value]] and units "
                                   f"a list of [op_row, a, b] or [op_row, a, b, count]: {e!r}") from e
        if not prog or len(prog) > 64:
            raise codec.CodecError(f"{what}: program must hold 1 to 64 entries")
        if not us or len(us) > 8:
            raise codec.CodecError(f"{what}: units must hold 1 to 8 entries")
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_alu(hs, prog, us, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "counts": st["counts"], "first": st["first"], "unknown": st["unknown"], "first_unknown": st["first_unknown"]}

    # ---- multi-limb integers: uint256 arithmetic and a b + c mod p over runs of limb rows, with the carries of the limb identity
    @_guard
    def worker_commit_wide(self, input_handles: Sequence[int], ops: Sequence[dict], usable: Optional[int] = None,
                           tail: Sequence[str] = ()):
        """Extension: multi-limb integer columns of the rows of the input_handles sets, computed and committed on the device as
        one new set.  A wide value is L consecutive rows, limb l in row first + l (little-endian), each cell reduced to its low
        b bits; 1 <= b <= 64, 1 <= L <= 8, b L <= 512.  ops: 1 to 8 objects {"kind", "bits", "limbs", "a", "b", "c", "q", "r",
        "m", "neg_c", "count"}: kind one of "add" "sub" "mul" "divmod" "mulmod" "carry"; a, c, q, r first rows (or null); b a
        first row, ["imm", value] or null; m the modulus; integers above 2^53 may be sent as decimal or 0x strings; count
        defaults to L (carry: 2 L - 1).  The rows of an op: add / sub: L limbs, then the carry / borrow; mul: low L limbs, high
        L limbs; divmod: quotient, remainder (2^W - 1 and a where b = 0); mulmod: r = (a b + d) mod m, then q, with d = c (or 0),
        or m - (c mod m) with neg_c; carry: the 2 L - 1 carries of the limb identity of that mulmod (b <= 56), a negative one
        as r_field - |x|.  usable and tail: as for worker_commit_int.  Returns the handle, the commitments, and per op
        `counts` / `first` (rows with a limb at or above 2^b) and `qover` / `first_qover` (mulmod: q at or above 2^W; carry:
        an inexact row).  Nothing here is a proof: the rows are prover data."""
        what = "worker_commit_wide"
        hs = _handles(input_handles)
        try:
            recs = []
            for op in ops:
                if not isinstance(op, dict):
                    raise ValueError(f"an op is an object: {op!r}")
                rec = dict(op)
                if isinstance(rec.get("b"), (list, tuple)):
                    rec["b"] = tuple(rec["b"])
                recs.append(rec)
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: ops must be a list of objects: {e!r}") from e
        if not recs:
            raise codec.CodecError(f"{what}: ops must not be empty")
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_wide(hs, recs, usable, tb)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments],
                "counts": st["counts"], "first": st["first"], "qover": st["qover"], "first_qover": st["first_qover"]}

    # ---- the hash chip: the Poseidon permutation (x^5, the caller's constants) per row, as a check, or as a round trace
    @_guard
    def worker_commit_poseidon(self, input_handles: Sequence[int], params: dict, units: Sequence[dict],
                               usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: Poseidon permutation columns of the rows of the input_handles sets, computed and committed on the device
        as one new set.  params: {"t", "full", "partial", "rc", "mds"}: the width t in [2, 8], R_F full rounds (even, 2 .. 16),
        R_P partial rounds (0 .. 128), the t (R_F + R_P) round constants round-major and the t x t matrix row-major; scalars
        below r as integers or decimal / 0x strings.  The library generates no constants.  Per round: s_i += rc[rho t + i]; s_i
        <- s_i^5 for every i in a full round (rho < R_F / 2 or rho >= R_F / 2 + R_P), for i = 0 only in a partial one; s <- M s.
        units: 1 to 8 objects.  {"mode": "row", "in": [t entries], "out": [state indices]} hashes every row t' < n (n = usable,
        or T) and commits one column per entry of out; with "expect": [rows] in place of the commitment it commits nothing and
        reports `mismatch`, the rows where an expected cell differs, and `first_mismatch`.  {"mode": "rounds", "in": [...],
        "period": P} with P >= R + 1 commits the t columns of the round trace: block b occupies rows [b P, b P + P), row b P +
        rho holds the state before round rho, row b P + R the output, the rest is 0.  An entry of in is a row index or ["imm",
        value].  usable and tail: as for worker_commit_derived.  Returns the handle (null when every unit is a check), the
        commitments, and per unit `perms`, `mismatch`, `first_mismatch`.  Nothing here is a proof: the columns are prover data
        and the argument is the caller's round gate in the quotient."""
        what = "worker_commit_poseidon"
        hs = _handles(input_handles)
        recs, par = self._unit_objects(what, units, ("in",), params=params), dict(params)
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_poseidon(hs, par, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments],
                "perms": st["perms"], "mismatch": st["mismatch"], "first_mismatch": st["first_mismatch"]}

    # ---- the hash chip a prover picks today: the Poseidon2 permutation, the units of worker_commit_poseidon
    @_guard
    def worker_commit_poseidon2(self, input_handles: Sequence[int], params: dict, units: Sequence[dict],
                                usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: Poseidon2 permutation columns of the rows of the input_handles sets, computed and committed on the device
        as one new set: worker_commit_poseidon with another permutation.  params: {"t", "full", "partial", "rc_full",
        "rc_partial", "diag"}: t in {2, 3, 4, 8}, R_F full rounds (even, 2 .. 16), R_P partial rounds (0 .. 128), the t R_F
        full-round constants round-major over both halves, the R_P partial-round constants, the t entries of diag; scalars below
        r as integers or decimal / 0x strings.  The library generates no constants.  s <- E(s); R_F / 2 full rounds (s_i +=
        rc_full[..]; s_i <- s_i^5 for every i; s <- E(s)); R_P partial rounds (s_0 += rc_partial[rho]; s_0 <- s_0^5; s <- I(s));
        R_F / 2 full rounds.  E: y_i = s_i + sum s_j at t = 2, 3; M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]] at t =
        4; circ(2 M4, M4) at t = 8.  I: y_i = diag_i s_i + sum s_j (the published mu_i enter as diag_i = mu_i - 1).  units: as
        for worker_commit_poseidon, except that a rounds unit needs P >= R + 2: row b P of block b holds the input, row b P + 1 +
        rho the state before round rho (row b P + 1 is E(input)), row b P + 1 + R the output, the rest is 0.  usable and tail:
        as for worker_commit_derived.  Returns the handle (null when every unit is a check), the commitments, and per unit
        `perms`, `mismatch`, `first_mismatch`.  Nothing here is a proof."""
        what = "worker_commit_poseidon2"
        hs = _handles(input_handles)
        recs, par = self._unit_objects(what, units, ("in",), params=params), dict(params)
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_poseidon2(hs, par, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments],
                "perms": st["perms"], "mismatch": st["mismatch"], "first_mismatch": st["first_mismatch"]}

    # ---- the hash chip's chains: a Poseidon sponge over a long message, a Merkle path, block after block along the column
    @_guard
    def worker_commit_poseidon_chain(self, input_handles: Sequence[int], params: dict, units: Sequence[dict],
                                     usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: Poseidon sponge and Merkle-path columns of the rows of the input_handles sets, computed and committed on
        the device as one new set.  params: as for worker_commit_poseidon (the caller's constants; none are generated).  units: 1
        to 4 objects, each a chain over blocks of P = period rows, b < floor(n / P) with n = usable, or T; a block cut by n is
        not started and its rows are 0.  Block b starts a segment when b = 0, when start is null, or when the start cell at row
        b P is not zero; otherwise it continues the block before.  {"mode": "sponge", "in": [t slots], "start": row or null,
        "period": P, "layout": ...}: a starting block's state is the slots at row b P; a continuing block's state is the output
        before it plus the cell where a slot is a row, and that output alone where it is an immediate, so a tag or capacity
        immediate enters once per message; with start null this is worker_commit_poseidon's rounds unit.  {"mode": "path",
        "cap": slot, "leaf": slot, "sib": [t - 2 rows], "pos": row, "digest": j, "start": row or null, "period": P, "layout":
        ...} (t >= 3, arity a = t - 1): state element 0 is cap, the child at position pos (the cell's whole integer; at or above
        a: position 0, counted in `bad_pos`) is the leaf on a starting block and element digest of the output before on a
        continuing one, the other children are the sib cells of row b P in their order.  "layout": "trace" (P >= R + 1) commits t
        columns laid out as a rounds unit lays them out; "flat" with "cols": [names among in0 .. in{t-1}, out0 .. out{t-1}]
        commits the named elements of the arranged state and of the output at row b P only (P = 1: one row per Merkle level).
        With "expect": row and "digest" in place of layout and cols a unit commits nothing: at the last block of each segment
        the digest is compared with the expect cell of that block's first row (`mismatch`, `first_mismatch`).  A slot is a row
        index or ["imm", value].  A segment is serial: it costs its length times one permutation's latency whatever the number
        of segments.  usable and tail: as for worker_commit_derived.  Returns the handle (null when every unit is a check), the
        commitments, and per unit `blocks`, `segments`, `bad_pos`, `first_bad_pos`, `mismatch`, `first_mismatch`.  Nothing here
        is a proof: the columns are prover data and the argument is the caller's gates."""
        what = "worker_commit_poseidon_chain"
        hs = _handles(input_handles)
        recs, par = self._unit_objects(what, units, ("in",), ("cap", "leaf"), params=params), dict(params)
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_poseidon_chain(hs, par, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments], **st}

    # ---- the bit-oriented hash chip: the SHA-256 compression per row, as a check, or as a chained round trace
    @_guard
    def worker_commit_sha256(self, input_handles: Sequence[int], units: Sequence[dict], usable: Optional[int] = None,
                             tail: Sequence[str] = ()):
        """Extension: SHA-256 compression columns of the rows of the input_handles sets, computed and committed on the device as
        one new set.  All values are 32-bit words: a source cell is its canonical integer reduced to its low 32 bits; a cell at
        or above 2^32 is reduced and counted (`counts`, `first`).  K and the standard initial value are built in.  units: 1 to 4
        objects.  {"mode": "row", "state": "iv" or [8 slots], "msg": [16 slots], "out": [word indices]} runs one compression per
        row t' < n (n = usable, or T) and commits word out[c] of the new chaining value as column c; with "expect": [rows] it
        commits nothing and reports `mismatch` and `first_mismatch`.  {"mode": "rounds", "msg": row, "start": row or null,
        "period": P >= 72, "iv": null or [8 words], "cols": [names]} commits the named columns (w, a, e, cw, ca, ce, sig0, sig1,
        sum0, maj, sum1, ch) of the round trace: block b occupies rows [b P, b P + P); rows 0 .. 3 hold the incoming chaining
        value, rows 4 .. 67 the 64 rounds with the schedule word read from msg at rows 4 .. 19, rows 68 .. 71 the feed-forward;
        a block starts a message when b = 0, start is null or its start cell at row b P is not zero, and continues the block
        before otherwise.  A slot is a row index or ["imm", v] with v < 2^32.  Padding is the caller's job.  usable and tail:
        as for worker_commit_derived.  Returns the handle (null when every unit is a check), the commitments, and per unit
        `blocks`, `messages`, `counts`, `first`, `mismatch`, `first_mismatch`.  Nothing here is a proof: the columns are prover
        data and the argument is the caller's gates plus the range lookups of words and carries."""
        what = "worker_commit_sha256"
        hs = _handles(input_handles)
        recs = self._unit_objects(what, units, ("state", "msg"))
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_sha256(hs, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments], **st}

    # ---- the Keccak chip: Keccak-f[1600] per row, as a check, or as a chained round trace of 64-bit lanes
    @_guard
    def worker_commit_keccak(self, input_handles: Sequence[int], units: Sequence[dict], usable: Optional[int] = None,
                             tail: Sequence[str] = ()):
        """Extension: Keccak-f[1600] permutation columns of the rows of the input_handles sets, computed and committed on the
        device as one new set.  All values are 64-bit lanes: a source cell is its canonical integer reduced to its low 64 bits;
        a cell at or above 2^64 is reduced and counted (`counts`, `first`).  The round constants and rotation offsets of FIPS
        202 are built in; lane (x, y) has the index x + 5 y, and a lane is the little-endian word of 8 message bytes.  units: 1
        to 4 objects.  {"mode": "row", "in": [25 slots], "out": [lane indices]} runs one permutation per row t' < n (n = usable,
        or T) and commits lane out[c] of the result as column c; with "expect": [rows] it commits nothing and reports `mismatch`
        and `first_mismatch`.  {"mode": "rounds", "msg": [5 rows], "rate": 1 .. 24, "start": row or null, "period": P >= 125,
        "cols": [names]} commits the named columns (a0 .. a4, p0 .. p4, d0 .. d4, t0 .. t4, b0 .. b4) of the round trace: block b
        occupies rows [b P, b P + P); rows 5 q + y hold round q, plane y, rows 120 .. 124 the outgoing state in the a columns;
        lane x + 5 y < rate absorbs the cell of msg[x] at block row y; a block starts a message when b = 0, start is null or its
        start cell at row b P is not zero, and continues the block before otherwise.  A slot is a row index or ["imm", v] with
        v < 2^64.  Padding is the caller's job.  usable and tail: as for worker_commit_derived.  Returns the handle (null when
        every unit is a check), the commitments, and per unit `perms`, `messages`, `counts`, `first`, `mismatch`,
        `first_mismatch`.  Nothing here is a proof: the columns are prover data and the argument is the caller's gates plus the
        range lookups of the lanes."""
        what = "worker_commit_keccak"
        hs = _handles(input_handles)
        recs = self._unit_objects(what, units, ("in",))
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_keccak(hs, recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments], **st}

    # ---- the non-native elliptic-curve chip: a / b mod p, affine point addition with the doubling, accumulator chains
    @_guard
    def worker_commit_ec(self, input_handles: Sequence[int], curve: dict, units: Sequence[dict], usable: Optional[int] = None,
                         tail: Sequence[str] = ()):
        """Extension: columns of elliptic-curve arithmetic over a foreign field, computed from the rows of the input_handles
        sets and committed on the device as one new set.  curve: {"bits": b, "limbs": L, "p": the odd modulus, 3 <= p < 2^(b L),
        b L <= 256, "a": the coefficient of y^2 = x^3 + a x + c, below p}; integers may be decimal or 0x strings.  A wide value
        is L consecutive rows of b bits, little-endian, named by its first row; an operand at or above p is reduced mod p; a
        row with a limb at or above 2^b or such an operand is counted (`counts`, `first`).  units: 1 to 4 objects.  {"mode":
        "div", "a": row, "b": row or ["imm", v], "out": true} commits a b^-1 mod p (0 and `singular` where b has no inverse).
        {"mode": "add", "x1", "y1", "x2", "y2": rows, "out": [names among lam, x3, y3]} commits the named values of the affine
        addition, the doubling where the points are equal; an exceptional row (opposite points, order two, no inverse) gives
        zeros and is counted in `singular`.  Either with "expect": [first rows] in place of out (add: three entries for lam, x3,
        y3, null: not compared) commits nothing and reports `mismatch` and `first_mismatch`.  {"mode": "chain", "px", "py":
        rows, "op": row, "cols": [names among ax, ay, lam]} commits the accumulator before each row's step and the step's
        lambda: op 0 holds, 1 loads (px, py), 2 adds it, 3 doubles, any other code holds and is counted in `unknown`; the
        accumulator is (0, 0) before row 0 and after an exceptional step; `segments` counts row 0 and the loads.  usable and
        tail: as for worker_commit_derived.  Returns the handle (null when every unit is a check), the commitments and the
        statistics per unit.  Nothing here is a proof: the columns are prover data and the argument is the caller's mulmod and
        carry gates over them plus the range lookups of the limbs."""
        what = "worker_commit_ec"
        hs = _handles(input_handles)
        recs = self._unit_objects(what, units, slots=("b",))
        if not isinstance(curve, dict):
            raise codec.CodecError(f"{what}: curve must be an object with bits, limbs, p and a")
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_ec(hs, dict(curve), recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments], **st}

    # ---- the native twisted-Edwards chip: point addition on a curve over the scalar field itself, accumulator chains
    @_guard
    def worker_commit_edwards(self, input_handles: Sequence[int], curve: dict, units: Sequence[dict],
                              usable: Optional[int] = None, tail: Sequence[str] = ()):
        """Extension: columns of arithmetic on a twisted Edwards curve over the scalar field itself (Jubjub, Bandersnatch),
        computed from the rows of the input_handles sets and committed on the device as one new set.  curve: {"a": A, "d": D},
        the coefficients of A x^2 + y^2 = 1 + D x^2 y^2, scalars below r as integers or decimal / 0x strings, not 0, not equal.
        The library generates no curve and ships no constant.  A coordinate is one cell; a slot is a row index or ["imm",
        value].  The law, with tau = D x1 x2 y1 y2: x3 = (x1 y2 + y1 x2) / (1 + tau), y3 = (y1 y2 - A x1 x2) / (1 - tau); the
        neutral element is (0, 1); there is no on-curve check; a row with tau = 1 or -1 is exceptional.  units: 1 to 4 objects.
        {"mode": "add", "x1", "y1", "x2", "y2": slots, "out": [names among x3, y3]} commits one row per name, in that order;
        an exceptional row gives zeros and is counted in `singular`.  With "expect": [row or null, row or null] in place of out
        it commits nothing and reports `mismatch` and `first_mismatch`.  {"mode": "chain", "px", "py": slots, "op": row,
        "cols": [names among ax, ay]} commits the accumulator before each row's step: op 0 holds, 1 loads (px, py), 2 adds it,
        3 doubles, 4 subtracts it, any other value holds and is counted in `unknown`; the accumulator is (0, 1) before row 0
        and after an exceptional step; `segments` counts row 0 and the loads.  usable and tail: as for worker_commit_derived.
        Returns the handle (null when every unit is a check), the commitments and the statistics per unit.  Nothing here is a
        proof: the columns are prover data and the argument is the caller's two addition gates under the op-code's selector."""
        what = "worker_commit_edwards"
        hs = _handles(input_handles)
        recs = self._unit_objects(what, units, slots=("x1", "y1", "x2", "y2", "px", "py"))
        if not isinstance(curve, dict):
            raise codec.CodecError(f"{what}: curve must be an object with a and d")
        usable, tb = self._layout(what, usable, tail)
        rs, st = self.engine.commit_edwards(hs, dict(curve), recs, usable, tb)
        return {"handle": None if rs is None else int(rs.handle),
                "commitments": [] if rs is None else [codec.g1_to_b64(c) for c in rs.commitments], **st}

    @staticmethod
    def shuffle_quotient_terms(z_row: int, input_rows: Sequence[int], shuffle_rows: Sequence[int], n_groups: int, width: int,
                               theta: str, gamma: str, coeff: str, active_row: Optional[int] = None,
                               input_sel: Optional[Sequence[Optional[int]]] = None,
                               shuffle_sel: Optional[Sequence[Optional[int]]] = None, ext_log: int = 2) -> list:
        """engine.shuffle_quotient_terms in the text form of worker_commit_quotient_ext / _zk / worker_quotient_part: the
        relation coeff * A * [z(wX) prod_g df_g - z(X) prod_g nf_g] as [coefficient, [[row, rot], ..]] terms.  The relations
        "z = 1 at row 0" and "z = 1 at row usable" stay the caller's gate terms over its rows L_0 / L_u."""
        from .engine import shuffle_quotient_terms

        terms = shuffle_quotient_terms(z_row, input_rows, shuffle_rows, n_groups, width, codec.fr_to_be32(theta),
                                       codec.fr_to_be32(gamma), codec.fr_to_be32(coeff), active_row, input_sel, shuffle_sel,
                                       ext_log)
        return [[codec.be32_to_fr(c), [[row, rot] for row, rot in fs]] for c, fs in terms]

    @_guard
    def worker_commit_quotient_zk(self, handles: Sequence[int], terms, perm=None, lookup=None, active_row=None,
                                  ext_log: int = 2, n_pieces: int = 3):
        """Extension: worker_commit_quotient_ext with the caller's active column: row active_row (1 on the usable rows, 0
        elsewhere) multiplies the permutation relation P1 and the lookup relation LK1, so that neither binds the blinding
        rows.  The permutation part then takes at most 2^ext_log - 1 wires, the lookup part at most 2^ext_log - 2 lookups.
        active_row = None is worker_commit_quotient_ext."""
        hs = _handles(handles)
        try:
            active_row = None if active_row is None else int(active_row)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"worker_commit_quotient_zk: active_row must be an integer or None: {e!r}") from e
        tt, pp, ll, ext_log, n_pieces = self._quotient_ext_parts("worker_commit_quotient_zk", terms, perm, lookup, ext_log,
                                                                 n_pieces)
        rs = self.engine.commit_quotient_zk(hs, tt, pp, ll, active_row, ext_log, n_pieces)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @staticmethod
    def _quotient_selectors(what: str, selectors):
        """per lookup null (no selector) or the row of the concatenation that holds q_l; None: the call without selectors"""
        if selectors is None:
            return None
        try:
            sel = [None if j is None else int(j) for j in selectors]
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"{what}: selectors must be a list of row indices or nulls: {e!r}") from e
        if any(j is not None and not 0 <= j < KZG_MAX_BATCH_OPEN for j in sel):
            raise codec.CodecError(f"{what}: a selector row index must be below {KZG_MAX_BATCH_OPEN}")
        return sel

    @_guard
    def worker_commit_quotient_sel(self, handles: Sequence[int], terms, perm=None, lookup=None, selectors=None, active_row=None,
                                   ext_log: int = 2, n_pieces: int = 3):
        """Extension: worker_commit_quotient_zk for lookups that are enabled on some rows only: selectors[l] is the row (of the
        concatenated sets) that holds q_l, the numerator of lookup l's fraction in the lookup relation, or null (the constant
        1) -- the rows worker_commit_multiplicities_sel and worker_commit_lookup_sum_sel read.  selectors = None is
        worker_commit_quotient_zk."""
        hs = _handles(handles)
        try:
            active_row = None if active_row is None else int(active_row)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"worker_commit_quotient_sel: active_row must be an integer or None: {e!r}") from e
        sel = self._quotient_selectors("worker_commit_quotient_sel", selectors)
        tt, pp, ll, ext_log, n_pieces = self._quotient_ext_parts("worker_commit_quotient_sel", terms, perm, lookup, ext_log,
                                                                 n_pieces)
        rs = self.engine.commit_quotient_sel(hs, tt, pp, ll, sel, active_row, ext_log, n_pieces)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @staticmethod
    def _quotient_ext_parts(what: str, terms, perm, lookup, ext_log, n_pieces):
        """the wire forms of worker_commit_quotient_ext's arguments -> the engine's (bytes and ints), scalars checked"""
        try:
            ext_log, n_pieces = int(ext_log), int(n_pieces)
            tt = [(codec.fr_to_be32(c), [(int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0) for f in fs])
                  for c, fs in terms]
            if any(isinstance(f, (tuple, list)) and len(f) != 2 for _, fs in terms for f in fs):
                raise ValueError("a factor is a row index or a [row, rot] pair")
            pp = None
            if perm is not None and len(perm["wires"]):   # (no wire: the part is off, as perm->k == 0 in C)
                pp = {"wires": [int(j) for j in perm["wires"]], "sigmas": [int(j) for j in perm["sigmas"]], "z": int(perm["z"]),
                      "shifts": [codec.fr_to_be32(x) for x in perm["shifts"]], "beta": codec.fr_to_be32(perm["beta"]),
                      "gamma": codec.fr_to_be32(perm["gamma"]), "alpha": codec.fr_to_be32(perm["alpha"])}
            ll = None
            if lookup is not None:
                ll = {"inputs": [int(j) for j in lookup["inputs"]], "table": [int(j) for j in lookup["table"]],
                      "mult": int(lookup["mult"]), "sum": int(lookup["sum"]), "width": int(lookup["width"]),
                      "theta": codec.fr_to_be32(lookup["theta"]), "beta": codec.fr_to_be32(lookup["beta"]),
                      "alpha": codec.fr_to_be32(lookup["alpha"])}
        except (TypeError, ValueError, KeyError, IndexError) as e:
            raise codec.CodecError(f"{what}: malformed terms, permutation or lookup part: {e!r}") from e
        scal = [c for c, _ in tt] + (pp["shifts"] + [pp["beta"], pp["gamma"], pp["alpha"]] if pp else []) + \
            ([ll["theta"], ll["beta"], ll["alpha"]] if ll else [])
        if any(int.from_bytes(x, "big") >= codec.R_MODULUS for x in scal):
            raise codec.CodecError(f"{what}: coefficients, shifts and challenges must be canonical scalars (< r)")
        return tt, pp, ll, ext_log, n_pieces

    # ---- the quotient in parts and the chained grand product: circuits that fit no single worker_commit_quotient_zk call
    @_guard
    def worker_quotient_part_sel(self, handles: Sequence[int], terms, perm=None, lookup=None, selectors=None, active_row=None,
                                 link=None, ext_log: int = 2, scale=None, acc=None):
        """Extension: worker_quotient_part with the lookup selectors of worker_commit_quotient_sel (selectors = None is
        worker_quotient_part)."""
        return self._quotient_part("worker_quotient_part_sel", handles, terms, perm, lookup,
                                   self._quotient_selectors("worker_quotient_part_sel", selectors), active_row, link, ext_log,
                                   scale, acc)

    @_guard
    def worker_quotient_part(self, handles: Sequence[int], terms, perm=None, lookup=None, active_row=None, link=None,
                             ext_log: int = 2, scale=None, acc=None):
        """Extension: one part of a quotient summed on the device over several calls.  handles, terms, perm, lookup and
        active_row as in worker_commit_quotient_zk, with this part's own row numbering; link: None or [prev_row, rot], which
        turns P2 into (z(X) - f_prev(w^rot X)) L_0(X), the chain relation of a chunked permutation; scale: None (1) or the
        scalar this part is multiplied by (the caller's power of alpha); acc: None (a new accumulator) or the handle an earlier
        part returned.  Returns {"acc": handle}.  worker_quotient_finish turns the accumulator into the pieces;
        worker_release_rows frees one that is not finished."""
        return self._quotient_part("worker_quotient_part", handles, terms, perm, lookup, None, active_row, link, ext_log, scale, acc)

    def _quotient_part(self, what, handles, terms, perm, lookup, sel, active_row, link, ext_log, scale, acc):
        hs = _handles(handles)
        try:
            active_row = None if active_row is None else int(active_row)
            ln = None if link is None else (int(link[0]), int(link[1]))
            if link is not None and len(link) != 2:
                raise ValueError("a link is a [prev_row, rot] pair")
            sc = None if scale is None else codec.fr_to_be32(scale)
            ah = None if acc is None else _handles([acc])[0]
        except (TypeError, ValueError, IndexError, KeyError) as e:
            raise codec.CodecError(f"{what}: active_row, link, scale and acc must be an integer, a [prev_row, rot] "
                                   f"pair, a scalar and a handle (or None): {e!r}") from e
        if sc is not None and int.from_bytes(sc, "big") >= codec.R_MODULUS:
            raise codec.CodecError(f"{what}: scale must be a canonical scalar (< r)")
        tt, pp, ll, ext_log, _ = self._quotient_ext_parts(what, terms, perm, lookup, ext_log, 1)
        if ln is not None and pp is None:
            raise codec.CodecError(f"{what}: a link needs a permutation part")
        accs = self._accs
        a = None
        if ah is not None:
            a = accs.get(ah)
            if a is None:
                raise codec.CodecError(f"{what}: acc names no live accumulator of this client")
        if sel is None:
            out = self.engine.quotient_part(hs, tt, pp, ll, active_row, ln, ext_log, sc, a)
        else:
            out = self.engine.quotient_part_sel(hs, tt, pp, ll, sel, active_row, ln, ext_log, sc, a)
        accs[int(out.handle)] = out
        return {"acc": int(out.handle)}

    @_guard
    def worker_quotient_finish(self, acc: int, n_pieces: int = 3):
        """Extension: the pieces of the quotient accumulated by worker_quotient_part, committed as a new set of n_pieces rows.
        Returns the new handle and the pieces' commitments; the accumulator is consumed.  When the quotient does not fit
        n_pieces rows (the constraints do not hold) nothing is created and the accumulator stays, to be released."""
        ah = _handles([acc])[0]
        try:
            n_pieces = int(n_pieces)
        except (TypeError, ValueError) as e:
            raise codec.CodecError(f"worker_quotient_finish: n_pieces must be an integer: {e!r}") from e
        if not 1 <= n_pieces <= 8:
            raise codec.CodecError(f"worker_quotient_finish: n_pieces = {n_pieces}, expected 1 .. 2^ext_log")
        accs = self._accs
        a = accs.get(ah)
        if a is None:
            raise codec.CodecError("worker_quotient_finish: acc names no live accumulator of this client")
        rs = self.engine.quotient_finish(a, n_pieces)
        accs.pop(ah, None)
        return {"handle": int(rs.handle), "commitments": [codec.g1_to_b64(c) for c in rs.commitments]}

    @_guard
    def worker_commit_grand_product_chain(self, wire_handles: Sequence[int], sigma_handles: Sequence[int], shifts: Sequence[str],
                                          beta: str, gamma: str, usable: int, tail: Sequence[str], start: str):
        """Extension: worker_commit_grand_product_zk whose z starts at `start` instead of 1: one chunk of a chained
        permutation.  The closing value z(w^usable) = start * prod N / prod D is the next chunk's start (1 after the last
        chunk when the permutation holds); the tail is untouched by start.  start must be canonical and not 0."""
        hw, hs, sh, ch = self._grand_product_args("worker_commit_grand_product_chain", wire_handles, sigma_handles, shifts,
                                                  (beta, gamma, start), "beta, gamma and start")
        if int.from_bytes(ch[2], "big") == 0:
            raise codec.CodecError("worker_commit_grand_product_chain: start must not be 0")
        usable, tb = self._blind("worker_commit_grand_product_chain", usable, tail)
        return self._with_closing(*self.engine.commit_grand_product_chain(hw, hs, sh, ch[0], ch[1], usable, tb, ch[2]))

    @_guard
    def worker_release_rows(self, handle: int):
        """Extension: frees a committed row set (or a quotient accumulator that was not finished)."""
        h = _handles([handle])[0]
        self.engine.release_rows(h)
        self._accs.pop(h, None)
        return {"released": True}

    @_guard
    def aggregate_commitments(self, commitments: Sequence[str]):
        """Pianist master aggregation: sum_i commit_i of the worker rows' commitments = the commitment of the whole
        bivariate polynomial (reference neurons/validator.py:196-198 distributes the rows; README.md:38 names the
        aggregation as the next milestone).  Points are decompressed and summed on the GPU."""
        raw = b"".join(codec.g1_from_b64(c) for c in commitments)
        return {"commitment": codec.g1_to_b64(self.engine.g1_sum_compressed(raw))}

    # ------------------------------------------------------------------ validator side (neurons/validator.py:58-104)
    @_guard
    def worker_verify(self, i: int, proof: str, alpha: str, eval: str, commitment: str):
        verify = getattr(self.engine, "verify", None)
        if verify is None:
            raise NotImplementedError("this engine has no verifier")
        ok = verify(self._slice(i), codec.g1_from_b64(proof), codec.fr_to_be32(alpha), codec.fr_to_be32(eval),
                    codec.g1_from_b64(commitment))
        return {"valid": bool(ok)}

    @_guard
    def worker_verify_open_batch(self, i: int, proof: str, alpha: str, gamma: str, evals: Sequence[str],
                                 commitments: Sequence[str]):
        """Extension: the pairing check of one worker_commit_open_batch answer."""
        vb = getattr(self.engine, "verify_open_batch", None)
        if vb is None:
            raise NotImplementedError("this engine has no batched-opening verifier")
        if len(evals) != len(commitments) or not 1 <= len(evals) <= KZG_MAX_BATCH_OPEN:
            raise codec.CodecError(f"worker_verify_open_batch: {len(evals)} evals for {len(commitments)} commitments")
        ok = vb(self._slice(i), [codec.g1_from_b64(c) for c in commitments], [codec.fr_to_be32(e) for e in evals],
                codec.fr_to_be32(alpha), codec.fr_to_be32(gamma), codec.g1_from_b64(proof))
        return {"valid": bool(ok)}

    @_guard
    def worker_verify_open_multi(self, i: int, proofs: Sequence[str], points: Sequence[str], opened: Sequence[Sequence[int]],
                                 gammas: Sequence[str], evals: Sequence[Sequence[str]], commitments: Sequence[str]):
        """Extension: the pairing check of one worker_commit_open_multi answer."""
        vm = getattr(self.engine, "verify_open_multi", None)
        if vm is None:
            raise NotImplementedError("this engine has no multi-point-opening verifier")
        m = len(points)
        if not (m == len(proofs) == len(opened) == len(gammas) == len(evals)) \
                or any(len(e) != len(r) for e, r in zip(evals, opened)) or not 1 <= len(commitments) <= KZG_MAX_BATCH_OPEN:
            raise codec.CodecError("worker_verify_open_multi: ragged points / proofs / opened rows / gammas / evals")
        ok = vm(self._slice(i), [codec.g1_from_b64(c) for c in commitments], [codec.fr_to_be32(x) for x in points], opened,
                [codec.fr_to_be32(x) for x in gammas], [[codec.fr_to_be32(e) for e in ev] for ev in evals],
                [codec.g1_from_b64(p) for p in proofs])
        return {"valid": bool(ok)}

    @_guard
    def worker_verify_open_lincomb(self, i: int, proofs: Sequence[str], points: Sequence[str],
                                   coeffs: Sequence[Sequence[str]], values: Sequence[str], commitments: Sequence[str]):
        """Extension: the pairing check of one worker_open_rows_lincomb answer against the k commitments of its rows."""
        vl = getattr(self.engine, "verify_open_lincomb", None)
        if vl is None:
            raise NotImplementedError("this engine has no caller-weighted-opening verifier")
        k, m = len(commitments), len(points)
        if not (1 <= m <= KZG_MAX_OPEN_POINTS and m == len(proofs) == len(coeffs) == len(values)) \
                or not 1 <= k <= KZG_MAX_BATCH_OPEN or any(len(c) != k for c in coeffs):
            raise codec.CodecError("worker_verify_open_lincomb: ragged points / proofs / coefficients / values / commitments")
        ok = vl(self._slice(i), [codec.g1_from_b64(c) for c in commitments], [codec.fr_to_be32(x) for x in points],
                [[codec.fr_to_be32(c) for c in cs] for cs in coeffs], [codec.fr_to_be32(v) for v in values],
                [codec.g1_from_b64(p) for p in proofs])
        return {"valid": bool(ok)}

    @_guard
    def worker_verify_open_shplonk(self, i: int, w: str, proof: str, u: str, points: Sequence[str],
                                   opened: Sequence[Sequence[int]], coeffs: Sequence[str], evals: Sequence[Sequence[str]],
                                   commitments: Sequence[str]):
        """Extension: the pairing check of one SHPLONK proof pair (w, proof) against the k commitments of its rows and the
        evaluations worker_eval_rows returned for the same points and row lists."""
        vs = getattr(self.engine, "verify_open_shplonk", None)
        if vs is None:
            raise NotImplementedError("this engine has no SHPLONK verifier")
        a, c = self._shplonk_args("worker_verify_open_shplonk", points, opened, coeffs)
        if len(commitments) != len(coeffs) or len(evals) != len(points) or any(len(e) != len(r) for e, r in zip(evals, opened)):
            raise codec.CodecError("worker_verify_open_shplonk: ragged commitments / coefficients / evaluations / row lists")
        ok = vs(self._slice(i), [codec.g1_from_b64(x) for x in commitments], a, opened, c,
                [[codec.fr_to_be32(e) for e in ev] for ev in evals], codec.g1_from_b64(w), codec.fr_to_be32(u),
                codec.g1_from_b64(proof))
        return {"valid": bool(ok)}

    @_guard
    def worker_verify_batch(self, indices: Sequence[int], proofs: Sequence[str], alpha: str, evals: Sequence[str],
                            commitments: Sequence[str], threads: int = 16):
        """Extension: every row of a validator step (they share alpha, neurons/validator.py:106-120) in ONE pairing check
        on a random linear combination of the rows.  {"valid": True} only when every row verifies; False does not say
        which row failed -- `validator.verify_all` then falls back to `worker_verify` row by row."""
        vb = getattr(self.engine, "verify_batch", None)
        if vb is None:
            raise NotImplementedError("this engine has no batch verifier")
        ok = vb([self._slice(i) for i in indices], [codec.g1_from_b64(p) for p in proofs], codec.fr_to_be32(alpha),
                [codec.fr_to_be32(e) for e in evals], [codec.g1_from_b64(c) for c in commitments], threads)
        return {"valid": bool(ok)}

    @_guard
    def fft(self, poly: Sequence[str], left: bool = True, inverse: bool = False):
        n = len(poly)
        want = 1 << (self.scale - self.machines_scale) if left else 1 << self.machines_scale
        if self.scale and n != want:
            raise codec.CodecError(f"fft(left={left}) expects {want} elements, got {n}")
        out = self.engine.ntt(codec.fr_list_to_be32(poly), bool(inverse))
        return {"poly": codec.be32_to_fr_list(out)}

    @_guard
    def eval(self, poly: Sequence[str], x: str):
        y = self.engine.eval(codec.fr_list_to_be32(poly), codec.fr_to_be32(x))
        return {"y": codec.be32_to_fr(y)}

    @_guard
    def fft_eval(self, poly: Sequence[str], x: str, left: bool = True, inverse: bool = True):
        """Extension: eval(fft(poly, left, inverse), x) in ONE call -- the validator's per-row challenge step (reference
        neurons/validator.py:115-118 makes the two calls; the 2^16 coefficients then cross the text codec twice)."""
        n = len(poly)
        want = 1 << (self.scale - self.machines_scale) if left else 1 << self.machines_scale
        if self.scale and n != want:
            raise codec.CodecError(f"fft(left={left}) expects {want} elements, got {n}")
        fast = getattr(self.engine, "ntt_eval_list", None)
        xb = codec.fr_to_be32(x)
        if fast and codec._wire:
            y = fast(poly, bool(inverse), xb)
        else:
            y = self.engine.eval(self.engine.ntt(codec.fr_list_to_be32(poly), bool(inverse)), xb)
        return {"y": codec.be32_to_fr(y)}

    @_guard
    def random_poly(self):
        """Bivariate polynomial as 2^machines_scale rows of 2^(scale-machines_scale) Fr (neurons/validator.py:67-75).
        Uniform on [0, r): getrandom + rejection, generated and encoded natively (csrc/wire_py.c) -- 2^24 strings at
        mainnet scale, which a Python loop needs ~40 s for, longer than the 30 s challenge deadline."""
        rows, T = 1 << self.machines_scale, 1 << (self.scale - self.machines_scale)
        if codec._wire is not None:
            return {"poly": codec._wire.random_fr_rows(rows, T)}
        return {"poly": [[codec.be32_to_fr(_random_fr()) for _ in range(T)] for _ in range(rows)]}

    @_guard
    def random_point(self):
        if codec._wire is not None:
            return {"point": codec._wire.random_fr_rows(1, 1)[0][0]}
        return {"point": codec.be32_to_fr(_random_fr())}


def _random_fr() -> bytes:
    return (secrets.randbelow(R_MODULUS)).to_bytes(32, "big")


def derive_taus(seed: int):
    """Deterministic (tau_x, tau_y) for synthetic SRS generation: SHA-256 counter stream reduced mod r."""
    import hashlib

    def h(tag: bytes) -> int:
        sb = seed.to_bytes(max(8, (seed.bit_length() + 7) // 8), "big")   # 8 bytes for seeds < 2^64 (fixture-stable)
        v = int.from_bytes(hashlib.sha256(b"kzg-mi355x-srs" + tag + sb).digest(), "big")
        return v % (R_MODULUS - 2) + 2

    return h(b"x"), h(b"y")
