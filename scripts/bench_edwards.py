"""The device-built twisted-Edwards columns (worker_commit_edwards' engine call) against the routes they replace, interleaved on
the same box, for T in {2^16, 2^20} over Jubjub in four shapes: the addition with both output rows; the check of x3 and y3
against the rows that unit committed; a chain of 512-row segments (a load, then adds, doublings and subtractions) with ax and
ay; a chain of ONE segment over the whole column (ONE lane walks every row; by default at 2^16 only and timed once).  The
operands are random field elements: the unit is arithmetic on pairs and asks for no curve point.  The source columns are
committed once, outside the timing.

  edwards   commit_edwards over the resident sets: the forward transforms, the phase-1 launch, ONE batched inversion, the finish
            launch, n_out inverse transforms, one MSM pass of n_out scalar sets (a check: one launch and nothing else).  Nothing
            row-sized crosses the host link
  route a   the rows computed on the host in Python integers (tests/edwards_ref.py), then commit_rows of the n_out 32-byte rows.
            The host part is TIMED OVER A SAMPLE of --host-rows rows, compared with the device's rows, and scaled to T (the loop
            is linear in the rows); route a = that + b
  route b   commit_rows of the same n_out precomputed 32-byte rows alone, upload included
  route c   for the check: the unit that commits x3 and y3

One JSON line per point with the ratios and the profiled stage split of the new call (`poly` holds the three launches and the
inversion).

    python scripts/bench_edwards.py [--rounds 3] [--reps 3] [--host-rows 2048] [--sizes 16,20] [--one-segment-sizes 16]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from tests import edwards_ref as er  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

CURVE = er.JUBJUB


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
        eng.gen_srs(0x0ED0A6 + lg, 0xFACADE, lg, 0)
        rng = np.random.default_rng(1000 * lg)
        raw = rng.integers(0, 256, (4, T, 32), dtype=np.uint8)
        raw[:, :, 0] = 0                                               # below 2^248: canonical
        cols = [raw[w].tobytes() for w in range(4)]
        codes = np.where(np.arange(T) % 512 == 0, 1, rng.integers(2, 5, T)).astype(np.uint8)
        one = codes.copy()
        one[1:][one[1:] == 1] = 2

        def op_row(c):
            b = np.zeros((T, 32), dtype=np.uint8)
            b[:, 31] = c
            return b.tobytes()

        A = eng.commit_rows(0, cols)
        O = eng.commit_rows(0, [op_row(codes)])
        O1 = eng.commit_rows(0, [op_row(one)])
        add = {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["x3", "y3"]}
        chain = {"mode": "chain", "px": 0, "py": 1, "op": 4, "cols": ["ax", "ay"]}
        E, _ = eng.commit_edwards([A], CURVE, [add])
        shapes = [("add x3, y3", [A], add), ("check x3, y3", [A, E], {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [4, 5]}),
                  ("chain, segments of 512", [A, O], chain)]
        if lg in one_sizes:
            shapes.append(("chain, one segment", [A, O1], chain))
        val = lambda w, t: int.from_bytes(cols[w][32 * t:32 * t + 32], "big")   # noqa: E731
        for name, sets, unit in shapes:
            check, single = "expect" in unit, name.endswith("one segment")
            rounds, reps = (1, 1) if single else (a.rounds, a.reps)

            def device():
                s, st = eng.commit_edwards(sets, CURVE, [unit])
                assert st["mismatch"] == [0] and st["unknown"] == [0]
                if s is None:
                    return []
                s.release()
                return s.commitments

            t0 = time.perf_counter()
            first = eng.commit_edwards([A] if check else sets, CURVE, [add if check else unit])[0]
            first_ms = (time.perf_counter() - t0) * 1e3
            rows = [eng.read_rows([first], c, 0, T, "fr")[0] for c in range(first.k)]
            first.release()
            got = lambda c, t: int.from_bytes(rows[c][32 * t:32 * t + 32], "big")   # noqa: E731
            # route a's host part over a sample, checked against the device's rows
            hr = min(a.host_rows, T)
            t0 = time.perf_counter()
            if unit["mode"] == "add":
                host = [er.add(CURVE, val(0, t), val(1, t), val(2, t), val(3, t))[:2] for t in range(hr)]
            else:
                acc, host, cs = er.NEUTRAL, [], (one if single else codes)
                for t in range(hr):
                    host.append(acc)
                    if cs[t] == 1:
                        acc = (val(0, t), val(1, t))
                    else:
                        q = acc if cs[t] == 3 else ((val(0, t) if cs[t] == 2 else -val(0, t) % er.R), val(1, t))
                        x3, y3, sing = er.add(CURVE, acc[0], acc[1], q[0], q[1])
                        acc = er.NEUTRAL if sing else (x3, y3)
            host_ms = (time.perf_counter() - t0) * 1e3 * T / hr
            for t in (0, hr // 2, hr - 1):
                assert (got(0, t), got(1, t)) == tuple(host[t]), (name, t)

            def route_b():
                s = eng.commit_rows(0, rows)
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
            line = {"metric": "edwards", "T_log2": lg, "case": name, "n_out": 0 if check else len(rows), "edwards_ms": round(md, 4),
                    "route_a_ms": round(host_ms + mb, 2), "route_a_host_ms_scaled": round(host_ms, 2), "route_a_host_rows_timed": hr,
                    "route_b_ms": round(mb, 4), "edwards_over_route_a": round(md / (host_ms + mb), 5),
                    "edwards_over_route_b": round(md / mb, 3), "edwards_rounds_ms": [round(x, 4) for x in td],
                    "route_b_rounds_ms": [round(x, 4) for x in tb], "edwards_stages_ms": st,
                    "poly_share": round(st.get("poly", 0.0) / max(sum(st.values()), 1e-9), 3), **ident}
            if check:                                   # route c: the unit that commits; route b is its committed rows
                def route_c():
                    s, _ = eng.commit_edwards([A], CURVE, [add])
                    s.release()

                route_c()
                tc = [timed(route_c, reps) for _ in range(rounds)]
                line.update(route_c_ms=round(median(tc), 4), edwards_over_route_c=round(md / median(tc), 3))
            print(json.dumps(line), flush=True)
        for s in (E, O, O1, A):
            s.release()
        eng.close()


if __name__ == "__main__":
    main()
