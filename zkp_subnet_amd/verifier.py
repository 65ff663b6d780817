"""Host-side opening verifier (pairing check) -- binding of the kzg_vk_* entry points.  No GPU involved: this is what
`Client.worker_verify` runs (reference neurons/validator.py:77-86)."""
from __future__ import annotations

import ctypes
from typing import Sequence

from . import _native
from ._native import KzgError


R_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def shplonk_finish_coeffs(points32: Sequence[bytes], opened: Sequence[Sequence[int]], coeffs32: Sequence[bytes],
                          u32: bytes) -> list:
    """The k + 1 scalars of SHPLONK's round B: lambda_j = c_j Z_{P \\ S_j}(u) for the k rows (S_j: the points p with j in
    opened[p]) and lambda_k = -Z_P(u) for h, the set kzg_rows_commit_shplonk made.  open_rows_lincomb over (rows, h) at the
    one point u with these proves the opening.  Pure host arithmetic; ValueError for u among the points, unequal lengths or a
    scalar that is not 32 canonical bytes."""
    if len(points32) != len(opened) or any(len(x) != 32 for x in list(points32) + list(coeffs32) + [u32]):
        raise ValueError("shplonk_finish_coeffs: one row list per point; points, coefficients and u of 32 bytes each")
    a = [int.from_bytes(x, "big") for x in points32]
    c = [int.from_bytes(x, "big") for x in coeffs32]
    u = int.from_bytes(u32, "big")
    if any(x >= R_MODULUS for x in a + c + [u]):
        raise ValueError("shplonk_finish_coeffs: scalars must be canonical (< r)")
    if u in a:
        raise ValueError("shplonk_finish_coeffs: u must not be one of the points")
    lam = []
    for j, cj in enumerate(c):
        for p, ap in enumerate(a):
            if j not in opened[p]:
                cj = cj * (u - ap) % R_MODULUS
        lam.append(cj)
    zp = 1
    for ap in a:
        zp = zp * (u - ap) % R_MODULUS
    lam.append(-zp % R_MODULUS)
    return [x.to_bytes(32, "big") for x in lam]


class Verifier:
    def __init__(self, handle):
        self._lib = _native.load()
        self._h = handle

    @classmethod
    def synthetic(cls, tau_x: int, factors: Sequence[int]) -> "Verifier":
        """Verifier key for a tau-derived SRS: [tau_x]_2 and [s0_k]_1 per resident slice (s0_k = L_i(tau_y))."""
        lib = _native.load()
        h = ctypes.c_void_p()
        s0 = b"".join(int(f).to_bytes(32, "big") for f in factors)
        rc = lib.kzg_vk_create_synthetic(int(tau_x).to_bytes(32, "big"), s0, len(s0) // 32, ctypes.byref(h))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_create_synthetic failed")
        return cls(h)

    @classmethod
    def from_points(cls, tau_g2_be192: bytes, li_g1_be96: bytes) -> "Verifier":
        lib = _native.load()
        h = ctypes.c_void_p()
        rc = lib.kzg_vk_create(tau_g2_be192, li_g1_be96, len(li_g1_be96) // 96, ctypes.byref(h))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_create failed: bad G2 / G1 key material")
        return cls(h)

    def export(self, n_slices: int) -> bytes:
        """192 B [tau_x]_2 followed by 96 B [L_i(tau_y)]_1 per slice: the contents of a `<setup>.vk` file."""
        out = ctypes.create_string_buffer(192 + 96 * n_slices)
        rc = self._lib.kzg_vk_export(self._h, out, len(out))
        if rc < 0:
            raise KzgError(rc, "kzg_vk_export failed")
        return out.raw[: 192 + 96 * rc]

    def verify(self, i: int, proof48: bytes, alpha32: bytes, eval32: bytes, commitment48: bytes) -> bool:
        if len(proof48) != 48 or len(commitment48) != 48:
            return False
        if len(alpha32) != 32 or len(eval32) != 32:          # the C side reads exactly 32 bytes of each
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify: alpha / eval must be 32 bytes")
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify(self._h, i, proof48, alpha32, eval32, commitment48, ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify: bad argument (index or non-canonical scalar)")
        return bool(ok.value)

    def verify_batch(self, indices: Sequence[int], proofs48: Sequence[bytes], alpha32: bytes, evals32: Sequence[bytes],
                     commitments48: Sequence[bytes], threads: int = 16) -> bool:
        """True only if EVERY (index, proof, eval, commitment) row verifies against the common alpha: one pairing check
        on a random linear combination of the rows (2^-128 soundness error).  False says nothing about which row."""
        n = len(indices)
        if not (n == len(proofs48) == len(evals32) == len(commitments48)):
            raise ValueError("verify_batch: ragged input")
        if len(alpha32) != 32 or any(len(e) != 32 for e in evals32):   # a short eval would have the C side read past
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify_batch: alpha / evals must be 32 bytes each")   # the joined buffer
        if any(len(p) != 48 for p in proofs48) or any(len(c) != 48 for c in commitments48):
            return False
        idx = (ctypes.c_uint32 * max(n, 1))(*indices)
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify_batch(self._h, n, idx, b"".join(proofs48), alpha32, b"".join(evals32),
                                           b"".join(commitments48), threads, ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify_batch: bad argument (index or non-canonical scalar)")
        return bool(ok.value)

    def verify_open_batch(self, i: int, commitments48: Sequence[bytes], evals32: Sequence[bytes], alpha32: bytes,
                          gamma32: bytes, proof48: bytes) -> bool:
        """One batched opening of k rows of slice i (kzg_vk_verify_open_batch):
        e(sum_j gamma^j C_j - (sum_j gamma^j y_j) L_i, [1]_2) == e(pi, [tau_x - alpha]_2)."""
        k = len(commitments48)
        if k != len(evals32):
            raise ValueError("verify_open_batch: one evaluation per commitment")
        if len(alpha32) != 32 or len(gamma32) != 32 or any(len(e) != 32 for e in evals32):
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify_open_batch: alpha / gamma / evals must be 32 bytes each")
        if len(proof48) != 48 or any(len(c) != 48 for c in commitments48):
            return False
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify_open_batch(self._h, i, k, b"".join(commitments48), b"".join(evals32), alpha32, gamma32,
                                                proof48, ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify_open_batch: bad argument (k, index or non-canonical scalar)")
        return bool(ok.value)

    def verify_open_multi(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                          opened: Sequence[Sequence[int]], gammas32: Sequence[bytes], evals32: Sequence[Sequence[bytes]],
                          proofs48: Sequence[bytes]) -> bool:
        """One multi-point opening of k rows of slice i (kzg_vk_verify_open_multi): opened[p] lists the rows opened at
        points32[p] (increasing), evals32[p] their evaluations there, proofs48[p] that point's proof; for every p
        e(sum_t gamma_p^t C_{j_t} - (sum_t gamma_p^t y_{j_t,p}) L_i, [1]_2) == e(pi_p, [tau_x - alpha_p]_2)."""
        k, m = len(commitments48), len(opened)
        if not (m == len(points32) == len(gammas32) == len(evals32) == len(proofs48)):
            raise ValueError("verify_open_multi: one point, gamma, evaluation list and proof per opened list")
        if any(len(e) != len(r) for e, r in zip(evals32, opened)):
            raise ValueError("verify_open_multi: one evaluation per opened row")
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN:
            raise KzgError(_native.KZG_E_ARG, f"kzg_vk_verify_open_multi: k = {k} outside [1, {_native.KZG_MAX_BATCH_OPEN}]")
        masks, _ = _native.open_masks(opened, k)
        flat = [e for ev in evals32 for e in ev]
        if any(len(x) != 32 for x in list(points32) + list(gammas32) + flat):
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify_open_multi: points / gammas / evals must be 32 bytes each")
        if any(len(c) != 48 for c in list(commitments48) + list(proofs48)):
            return False
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify_open_multi(self._h, i, k, b"".join(commitments48), m, b"".join(points32), masks,
                                                b"".join(gammas32), b"".join(flat), b"".join(proofs48), ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify_open_multi: bad argument (k, m, mask, index or non-canonical scalar)")
        return bool(ok.value)

    def verify_open_lincomb(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                            coeffs: Sequence[Sequence[bytes]], values32: Sequence[bytes], proofs48: Sequence[bytes]) -> bool:
        """One caller-weighted opening of k rows of slice i (kzg_vk_verify_open_lincomb): coeffs[p] holds the k scalars of
        point p; for every p  e(sum_j coeffs[p][j] C_j - v_p L_i, [1]_2) == e(pi_p, [tau_x - alpha_p]_2)."""
        k, m = len(commitments48), len(points32)
        if not (m == len(coeffs) == len(values32) == len(proofs48)) or any(len(c) != k for c in coeffs):
            raise ValueError("verify_open_lincomb: one point, k coefficients, value and proof per point")
        if k == 0 or k > _native.KZG_MAX_BATCH_OPEN or m == 0 or m > _native.KZG_MAX_OPEN_POINTS:
            raise KzgError(_native.KZG_E_ARG, f"kzg_vk_verify_open_lincomb: k = {k}, m = {m} outside the limits")
        flat = [c for cs in coeffs for c in cs]
        if any(len(x) != 32 for x in list(points32) + flat + list(values32)):
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify_open_lincomb: points / coefficients / values must be 32 bytes")
        if any(len(c) != 48 for c in list(commitments48) + list(proofs48)):
            return False
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify_open_lincomb(self._h, i, k, b"".join(commitments48), m, b"".join(points32),
                                                  b"".join(flat), b"".join(values32), b"".join(proofs48), ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify_open_lincomb: bad argument (k, m, all-zero point, index or non-canonical scalar)")
        return bool(ok.value)

    def verify_open_shplonk(self, i: int, commitments48: Sequence[bytes], points32: Sequence[bytes],
                            opened: Sequence[Sequence[int]], coeffs32: Sequence[bytes], evals32: Sequence[Sequence[bytes]],
                            w48: bytes, u32: bytes, proof48: bytes) -> bool:
        """One SHPLONK opening of k rows of slice i (kzg_vk_verify_open_shplonk): opened[p] lists the rows opened at
        points32[p] (increasing), evals32[p] their evaluations there (eval_rows' shape), coeffs32 the k row scalars c_j,
        (w48, proof48) the proof pair and u32 the point of round B.  Two pairings whatever the number of points."""
        k, m = len(commitments48), len(points32)
        if not (m == len(opened) == len(evals32)) or len(coeffs32) != k:
            raise ValueError("verify_open_shplonk: one row list and evaluation list per point, one coefficient per commitment")
        if any(len(e) != len(r) for e, r in zip(evals32, opened)):
            raise ValueError("verify_open_shplonk: one evaluation per opened row")
        if k == 0 or k > _native.KZG_MAX_SHPLONK_ROWS:
            raise KzgError(_native.KZG_E_ARG, f"kzg_vk_verify_open_shplonk: k = {k} outside [1, {_native.KZG_MAX_SHPLONK_ROWS}]")
        masks, _ = _native.shplonk_masks(opened, k)
        flat = [e for ev in evals32 for e in ev]
        if any(len(x) != 32 for x in list(points32) + list(coeffs32) + flat + [u32]):
            raise KzgError(_native.KZG_E_ARG, "kzg_vk_verify_open_shplonk: points / coefficients / evals / u must be 32 bytes")
        if any(len(c) != 48 for c in list(commitments48) + [w48, proof48]):
            return False
        ok = ctypes.c_int(0)
        rc = self._lib.kzg_vk_verify_open_shplonk(self._h, i, k, b"".join(commitments48), m, b"".join(points32), masks,
                                                  b"".join(coeffs32), b"".join(flat), w48, u32, proof48, ctypes.byref(ok))
        if rc != 0:
            raise KzgError(rc, "kzg_vk_verify_open_shplonk: bad argument (k, m, equal points, u among the points, a mask, a "
                               "nonzero coefficient on an unopened row, index or non-canonical scalar)")
        return bool(ok.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.kzg_vk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
