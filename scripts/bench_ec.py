"""The device-built elliptic-curve columns (worker_commit_ec's engine call) against the routes they replace, interleaved on the
same box, for T in {2^16, 2^20} over secp256k1 in 64-bit limbs (b = 64, L = 4) in five shapes: the addition with all 12 output
rows; the division x1 / x2 (4 rows); the check of a doubling's x3 and y3 (8 operand rows serving twice, 8 expected rows); a chain
of 512-row segments (a load, then adds and doublings) with ax, ay and lam; a chain of ONE segment over the whole column (ONE lane
walks every row; by default at 2^16 only and timed once: it takes minutes at 2^20).  The source columns are committed once,
outside the timing.

  ec        commit_ec over the resident sets: the forward transforms, ONE launch, n_out inverse transforms, one MSM pass of n_out
            scalar sets (a check: neither).  Nothing row-sized crosses the host link
  route a   the rows computed on the host in Python integers (tests/ec_ref.py), then commit_rows_typed of the n_out u64 limb
            columns.  The host part is TIMED OVER A SAMPLE of --host-rows rows, compared with the device's rows, and scaled to T
            (the loop is linear in the rows); route a = that + b
  route b   commit_rows_typed of the same n_out precomputed u64 limb columns alone, upload included
  route c   for the check: the unit that commits x3 and y3

One JSON line per point with the ratios, the profiled stage split of the new call (`poly` holds the kernel) and the inversions
per second that the kernel's share amounts to.

    python scripts/bench_ec.py [--rounds 3] [--reps 3] [--host-rows 2048] [--sizes 16,20] [--one-segment-sizes 16]"""
import argparse
import array
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from tests import ec_ref as er  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

CURVE, L = er.SECP, 4
NAMES = ["lam", "x3", "y3"]


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-rows", type=int, default=2048, help="rows of route a's host part that are timed")
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--one-segment-sizes", default="16")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    one_sizes = [int(x) for x in a.one_segment_sizes.split(",") if x]
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x0EC0A6 + lg, 0xFACADE, lg, 0)
        rng = np.random.default_rng(1000 * lg)
        # four operands below p: the top limb is below 2^63
        limbs = [rng.integers(0, 1 << (63 if l % 4 == 3 else 64), T, dtype=np.uint64) for l in range(16)]
        cols = [array.array("Q", c.tolist()) for c in limbs]
        ops = np.where(np.arange(T) % 512 == 0, 1, rng.integers(2, 4, T)).astype(np.uint64)
        one = ops.copy()
        one[1:][one[1:] == 1] = 2
        A = eng.commit_rows_typed(0, cols)
        A8 = eng.commit_rows_typed(0, cols[:8])                        # x1, y1 alone: a call's sets hold at most 16 rows in all
        O = eng.commit_rows_typed(0, [array.array("Q", ops.tolist())])
        O1 = eng.commit_rows_typed(0, [array.array("Q", one.tolist())])
        add = {"mode": "add", "x1": 0, "y1": 4, "x2": 8, "y2": 12, "out": NAMES}
        div = {"mode": "div", "a": 0, "b": 8, "out": True}
        dbl = {"mode": "add", "x1": 0, "y1": 4, "x2": 0, "y2": 4, "out": ["x3", "y3"]}
        chain = {"mode": "chain", "px": 0, "py": 4, "op": 8, "cols": ["ax", "ay", "lam"]}
        E, _ = eng.commit_ec([A], CURVE, [dbl])
        shapes = [("add 12 rows", [A], add), ("div 4 rows", [A], div),
                  ("check x3, y3 of a doubling", [A8, E], {"mode": "add", "x1": 0, "y1": 4, "x2": 0, "y2": 4, "expect": [None, 8, 12]}),
                  ("chain, segments of 512", [A8, O], chain)]
        if lg in one_sizes:
            shapes.append(("chain, one segment", [A8, O1], chain))
        val = lambda first, t: sum(cols[first + l][t] << (64 * l) for l in range(4))   # noqa: E731
        for name, sets, unit in shapes:
            check, single = "expect" in unit, name.endswith("one segment")
            rounds, reps = (1, 1) if single else (a.rounds, a.reps)

            def device():
                s, st = eng.commit_ec(sets, CURVE, [unit])
                assert st["mismatch"] == [0] and st["counts"] == [0] and st["unknown"] == [0]
                if s is None:
                    return []
                s.release()
                return s.commitments

            t0 = time.perf_counter()
            first = eng.commit_ec([A] if check else sets, CURVE, [dbl if check else unit])[0]
            first_ms = (time.perf_counter() - t0) * 1e3
            rows = [array.array("Q", eng.read_rows([first], c, 0, T, "u64")[0]) for c in range(first.k)]
            first.release()
            got = lambda c, t: sum(rows[4 * c + l][t] << (64 * l) for l in range(4))   # noqa: E731
            # route a's host part over a sample, checked against the device's rows
            hr = min(a.host_rows, T)
            t0 = time.perf_counter()
            if unit["mode"] == "div":
                host = [(er.div(CURVE, val(0, t), val(8, t))[0],) for t in range(hr)]
            elif unit["mode"] == "add":
                second = (0, 4) if check else (8, 12)
                host = [er.add(CURVE, val(0, t), val(4, t), val(second[0], t), val(second[1], t))[:3] for t in range(hr)]
                if check:
                    host = [h[1:] for h in host]
            else:
                acc, host, codes = (0, 0), [], (one if single else ops)
                for t in range(hr):
                    lam, nxt = 0, acc
                    if codes[t] == 1:
                        nxt = (val(0, t), val(4, t))
                    else:
                        q = (val(0, t), val(4, t)) if codes[t] == 2 else acc
                        lam, x3, y3, _ = er.add(CURVE, acc[0], acc[1], q[0], q[1])
                        nxt = (x3, y3)
                    host.append((acc[0], acc[1], lam))
                    acc = nxt
            host_ms = (time.perf_counter() - t0) * 1e3 * T / hr
            for t in (0, hr // 2, hr - 1):
                assert tuple(got(c, t) for c in range(len(host[t]))) == tuple(host[t]), (name, t)

            def route_b():
                s = eng.commit_rows_typed(0, rows)
                s.release()
                return s.commitments

            def timed(f, n):
                samples = []
                for _ in range(n):
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

            if single:   # one call is the measurement: the first one above, and the profiled one below
                assert route_b()
                td, tb = [first_ms], [timed(route_b, a.reps)]
            else:
                warm = device()                             # (also the warm-up)
                assert check or warm == route_b()
                td, tb = [], []
                for _ in range(rounds):                     # interleaved: the routes see the same clock and thermal state
                    td.append(timed(device, reps))
                    tb.append(timed(route_b, reps))
            md, mb = median(td), median(tb)
            st = stages(device)
            line = {"metric": "ec", "T_log2": lg, "case": name, "n_out": 0 if check else len(rows), "ec_ms": round(md, 4),
                    "route_a_ms": round(host_ms + mb, 2), "route_a_host_ms_scaled": round(host_ms, 2), "route_a_host_rows_timed": hr,
                    "route_b_ms": round(mb, 4), "ec_over_route_a": round(md / (host_ms + mb), 5), "ec_over_route_b": round(md / mb, 3),
                    "ec_rounds_ms": [round(x, 4) for x in td], "route_b_rounds_ms": [round(x, 4) for x in tb], "ec_stages_ms": st,
                    "poly_share": round(st.get("poly", 0.0) / max(sum(st.values()), 1e-9), 3),
                    "inversions_per_s": round(T / max(st.get("poly", 0.0), 1e-9) * 1e3), **ident}
            if check:                                   # route c: the unit that commits; route b is its committed columns
                def route_c():
                    s, _ = eng.commit_ec([A], CURVE, [dbl])
                    s.release()

                route_c()
                tc = [timed(route_c, reps) for _ in range(rounds)]
                line.update(route_c_ms=round(median(tc), 4), ec_over_route_c=round(md / median(tc), 3))
            print(json.dumps(line), flush=True)
        for s in (E, O, O1, A8, A):
            s.release()
        eng.close()


if __name__ == "__main__":
    main()
