"""Plain helpers shared by the test modules and the `*_ref.py` references: scalars as 32 big-endian bytes and back.  Nothing
here needs a device (the `hip` engine factory fixture lives in tests/conftest.py, the row-set helpers of the `-m gpu` modules
in tests/gpu_rows.py)."""
import os

from oracle.bls12_381 import R

H = bytes.fromhex
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_scalars_bytes(n, seed):
    import numpy as np                      # here, so that the CPU tests and references import this module without it

    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F                       # < 2^254 < r: canonical
    return raw.tobytes()


def be(v):
    return (v % R).to_bytes(32, "big")


def val(b):
    return int.from_bytes(b, "big")


def ints(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def row_bytes(vals):
    return b"".join(be(v) for v in vals)
