"""The device-built multi-limb integer columns (worker_commit_wide's engine call) against the routes they replace, interleaved on
the same box, for T in {2^16, 2^20} and four shapes: the 512-bit product of two uint256 at b = 64, L = 4 (8 rows); r and q of
a b mod secp256k1's p at b = 32, L = 8 (16 rows); the carry columns of such a limb identity at b = 32, L = 4 against a 128-bit
modulus (7 rows: a call reads at most 16 rows, and a, b, q, r at L = 8 would be 32); r and q of a b mod BLS12-381's p at b = 64,
L = 6 (12 rows).  The source columns are committed once, outside the timing.

  wide     commit_wide over the resident sets: one forward transform per distinct limb row, ONE launch, n_out inverse transforms,
           one MSM pass of n_out scalar sets.  Nothing row-sized crosses the host link
  route a  the rows computed on the host in Python integers, packed to 32-byte scalars, then commit_rows of the n_out rows
  route b  commit_rows of the same n_out (precomputed) rows alone, upload included

One JSON line per point with both ratios and the profiled stage split of the new call (`poly` holds the kernel).

    python scripts/bench_wide.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

SECP256K1_P = (1 << 256) - (1 << 32) - 977
BLS12_381_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
M128 = (1 << 128) - 159
# (name, b, L, modulus or None, kind)
CASES = [("mul uint256 b64 L4", 64, 4, None, "mul"), ("mulmod secp256k1 b32 L8", 32, 8, SECP256K1_P, "mulmod"),
         ("carry b32 L4 m128", 32, 4, M128, "carry"), ("mulmod bls12-381 b64 L6", 64, 6, BLS12_381_P, "mulmod")]


def limbs(vals, b, L):
    return [[(v >> (b * l)) & ((1 << b) - 1) for v in vals] for l in range(L)]


def host_rows(av, bv, b, L, m, kind):
    """the op's output rows from the wide values, on the host"""
    if kind == "mul":
        return limbs([x * y for x, y in zip(av, bv)], b, 2 * L)
    t = [x * y for x, y in zip(av, bv)]
    q, r = [x // m for x in t], [x % m for x in t]
    if kind == "mulmod":
        return limbs(r, b, L) + limbs(q, b, L)
    R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    A, B, Q, Rm, Mm = limbs(av, b, L), limbs(bv, b, L), limbs(q, b, L), limbs(r, b, L), [(m >> (b * l)) & ((1 << b) - 1) for l in range(L)]
    rows = [[0] * len(av) for _ in range(2 * L - 1)]
    for t_ in range(len(av)):
        carry = 0
        for k in range(2 * L - 1):
            s = carry + sum(A[i][t_] * B[k - i][t_] - Q[i][t_] * Mm[k - i] for i in range(L) if 0 <= k - i < L)
            if k < L:
                s -= Rm[k][t_]
            carry = s >> b
            rows[k][t_] = carry % R
    return rows


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-reps", type=int, default=1, help="calls per timed sample of route a")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x51DE + lg, 0xFACADE, lg, 0)
        for name, b, L, m, kind in CASES:
            rnd = random.Random(1000 * lg + b + L)
            top = m if m else 1 << (b * L)
            av, bv = [rnd.randrange(top) for _ in range(T)], [rnd.randrange(top) for _ in range(T)]
            cols = limbs(av, b, L) + limbs(bv, b, L)
            if kind == "carry":
                cols += limbs([x * y % m for x, y in zip(av, bv)], b, L) + limbs([x * y // m for x, y in zip(av, bv)], b, L)
                op = dict(kind="carry", bits=b, limbs=L, a=0, b=L, r=2 * L, q=3 * L, m=m)
            else:
                op = dict(kind=kind, bits=b, limbs=L, a=0, b=L, count=2 * L)
                if m:
                    op["m"] = m
            A = eng.commit_rows(0, [pack(c) for c in cols])
            rows = [pack(r) for r in host_rows(av, bv, b, L, m, kind)]

            def device():
                s, st = eng.commit_wide([A], [op])
                s.release()
                assert not any(st["counts"]) and not any(st["qover"])
                return s.commitments

            def route_a():
                s = eng.commit_rows(0, [pack(r) for r in host_rows(av, bv, b, L, m, kind)])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def timed(f, reps):
                samples = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                return median(samples) * 1e3

            def stages(f):
                eng._chk(lib.kzg_set_profiling(eng._h, 1))
                try:
                    f()
                    tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                    eng._chk(lib.kzg_get_timings(eng._h, tms, len(tms)))
                finally:
                    eng._chk(lib.kzg_set_profiling(eng._h, 0))
                return {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v}

            assert device() == route_b()                # (also the warm-up; route a commits the same rows)
            device()
            td, ta, tb = [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                ta.append(timed(route_a, a.host_reps))
                tb.append(timed(route_b, a.reps))
            md, ma, mb = median(td), median(ta), median(tb)
            print(json.dumps({"metric": "wide", "T_log2": lg, "case": name, "n_out": len(rows), "wide_ms": round(md, 4),
                              "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4),
                              "wide_over_route_a": round(md / ma, 4), "wide_over_route_b": round(md / mb, 3),
                              "wide_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              "route_b_rounds_ms": [round(x, 4) for x in tb], "wide_stages_ms": stages(device), **ident}),
                  flush=True)
            A.release()
        eng.close()


if __name__ == "__main__":
    main()
