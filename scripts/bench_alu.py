"""The ALU column with an op-code column (worker_commit_alu's engine call) against the routes it replaces, interleaved on the
same box, for T in {2^16, 2^20}.  The source columns are committed once, outside the timing.

  alu      commit_alu over the resident set: one forward transform per distinct source row (the op-code column among them), ONE
           launch, n_out inverse transforms, one MSM pass of n_out scalar sets
  route b  commit_rows of the same n_out precomputed rows, upload included
  route c  commit_int with the same single kind (constant op-code shapes only): the op-code column's transform and its cell
           load are the whole difference
  route d  what the header recommended before this call, for the four-kind program add / xor / ltu / srl at w = 32: one
           commit_int per candidate (add, xor, sub with its borrow, split at the shift b mod 32) and the commit_expr that
           selects one of them per row through the caller's four selector columns (committed outside the timing)

Shapes: a constant op-code column of add with its carry and of divmod (two rows each, routes b and c); the four-kind program on
a random op-code column (one row, routes b and d); all 23 kinds at w = 32 on a constant and on a random op-code column (two
rows, route b), whose profiled `poly` stage is the kernel without and with divergence.  One JSON line per point, stamped with
the library identity like bench.py's lines.

    python scripts/bench_alu.py [--rounds 3] [--reps 3] [--sizes 16,20]"""
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
from tests import alu_ref as aref  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

W = 32
FOUR = [("add", W), ("xor", W), ("ltu", W), ("srl", W)]
ALL = [(k, W) for k in aref.KINDS]


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample (the median is reported)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    one = (1).to_bytes(32, "big")
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0xA1C + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        # rows of A: 0 a, 1 b (a zero in every 64th cell), 2 op = 0, 3 op random over 4 kinds, 4 op random over 23 kinds, 5 op = 6
        # (divmod), 6 op = 3 (add), 7 b mod 32; the set B: the selector columns of the four kinds
        xs = [rnd.randrange(1 << W) for _ in range(T)]
        ys = [0 if t % 64 == 17 else rnd.randrange(1, 1 << W) for t in range(T)]
        op4 = [rnd.randrange(4) for _ in range(T)]
        op23 = [rnd.randrange(23) for _ in range(T)]
        cols = [xs, ys, [0] * T, op4, op23, [6] * T, [3] * T, [y % W for y in ys]]
        A = eng.commit_rows(0, [pack(c) for c in cols])
        B = eng.commit_rows(0, [pack([int(c == k) for c in op4]) for k in range(4)])
        shapes = [("add + carry, constant op", ALL, (6, 0, 1, 2), ("add", W, 0, 1, 2)),
                  ("divmod, constant op", ALL, (5, 0, 1, 2), ("divmod", W, 0, 1, 2)),
                  ("4 kinds, random op, 1 row", FOUR, (3, 0, 1), None),
                  ("23 kinds, constant op", ALL, (2, 0, 1, 2), None),
                  ("23 kinds, random op", ALL, (4, 0, 1, 2), None)]
        for name, program, unit, int_op in shapes:
            rows = [pack(r) for r in aref.alu_columns(cols, program, [unit])[0]]

            def device():
                s, st = eng.commit_alu([A], program, [unit])
                s.release()
                assert st["unknown"] == [0]
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def route_c():
                s, _, _ = eng.commit_int([A], [int_op])
                s.release()
                return s.commitments

            def route_d():
                cand = []
                for op in (("add", W, 0, 1), ("xor", W, 0, 1), ("sub", W, 0, 1, 2), ("split", W, 0, 7)):
                    cand.append(eng.commit_int([A], [op])[0])
                # rows behind B's four selectors: 4 add, 5 xor, 6 difference, 7 borrow, 8 a >> s
                s = eng.commit_expr([B] + cand, [([(one, [0, 4]), (one, [1, 5]), (one, [2, 7]), (one, [3, 8])],)])[0]
                for c in cand + [s]:
                    c.release()
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

            routes = {"alu": device, "route_b": route_b}
            if int_op:
                routes["route_c"] = route_c
            if program is FOUR:
                routes["route_d"] = route_d
            want = device()                             # (also the warm-up: buffers, twiddles)
            for f in routes.values():
                assert f() == want                      # every route commits the same rows
            times = {k: [] for k in routes}
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                for k, f in routes.items():
                    times[k].append(timed(f, a.reps))
            med = {k: median(v) for k, v in times.items()}
            line = {"metric": "alu", "T_log2": lg, "case": name, "n_out": len(rows)}
            for k in routes:
                line[k + "_ms"] = round(med[k], 4)
                line[k + "_rounds_ms"] = [round(x, 4) for x in times[k]]
                if k != "alu":
                    line["alu_over_" + k] = round(med["alu"] / med[k], 3)
            print(json.dumps({**line, "alu_stages_ms": stages(device), **ident}), flush=True)
        A.release()
        B.release()
        eng.close()


if __name__ == "__main__":
    main()
