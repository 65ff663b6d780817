"""The device-built Poseidon columns (worker_commit_poseidon's engine call) against the routes they replace, interleaved on the
same box, for T in {2^16, 2^20} at t = 3, R_F = 8, R_P = 57 (seeded random constants, a Cauchy matrix) in three shapes: a row
unit with one output column; a rounds unit with P = 128 (three columns, T / 128 permutations); a check of one expected column.
The three source columns are committed once, outside the timing.

  poseidon  commit_poseidon over the resident set: three forward transforms, ONE launch, n_out inverse transforms, one MSM pass
            of n_out scalar sets (a check: neither).  Nothing row-sized crosses the host link
  route a   the rows computed on the host in Python integers, packed to 32-byte scalars, then commit_rows of the n_out rows.
            828 modular products per permutation in Python make 2^20 of them a quarter of an hour, so the host part is TIMED
            OVER A SAMPLE of --host-perms permutations, compared cell by cell with the device's rows, and scaled to the shape's
            number of permutations (the loop is linear in them); route a = that + route b
  route b   commit_rows of the same n_out precomputed rows alone, upload included (the rows are read back from the device set
            once, outside the timing)
  route c   for the check: the row unit that commits (shape 1)

One JSON line per point with the ratios and the profiled stage split of the new call (`poly` holds the kernel).

    python scripts/bench_poseidon.py [--rounds 3] [--reps 3] [--host-perms 2048] [--sizes 16,20]"""
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
T_W, FULL, PARTIAL, PERIOD = 3, 8, 57, 128


def make_params(seed):
    rnd = random.Random(seed)
    return {"t": T_W, "full": FULL, "partial": PARTIAL, "rc": [rnd.randrange(R) for _ in range(T_W * (FULL + PARTIAL))],
            "mds": [pow(1 + i + T_W + j, R - 2, R) for i in range(T_W) for j in range(T_W)]}


def host_trace(params, s):
    """the states before every round and behind the last, in Python integers"""
    t, rc, M, half = params["t"], params["rc"], params["mds"], params["full"] // 2
    out = [list(s)]
    for rho in range(params["full"] + params["partial"]):
        full = rho < half or rho >= half + params["partial"]
        u = [(s[i] + rc[rho * t + i]) % R for i in range(t)]
        x = [pow(u[i], 5, R) if (full or i == 0) else u[i] for i in range(t)]
        s = [sum(M[i * t + j] * x[j] for j in range(t)) % R for i in range(t)]
        out.append(s)
    return out


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-perms", type=int, default=2048, help="permutations of route a's host part that are timed")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    params = make_params(0x905E1D0)
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x905E + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(T_W)]
        A = eng.commit_rows(0, [pack(c) for c in cols])
        row_unit = {"mode": "row", "in": [0, 1, 2], "out": [0]}
        rounds_unit = {"mode": "rounds", "in": [0, 1, 2], "period": PERIOD}
        E, _ = eng.commit_poseidon([A], params, [row_unit])          # the expected column of the check, resident
        shapes = [("row 1 output", [A], [row_unit], T), ("rounds P=128 3 columns", [A], [rounds_unit], T // PERIOD),
                  ("check 1 column", [A, E], [dict(row_unit, expect=[3])], T)]
        for name, sets, units, perms in shapes:
            check = "expect" in units[0]

            def device():
                s, st = eng.commit_poseidon(sets, params, units)
                assert st["perms"] == [perms] and st["mismatch"] == [0]
                if s is None:
                    return []
                s.release()
                return s.commitments

            first = eng.commit_poseidon([A], params, [row_unit] if check else units)[0]
            rows = [eng.read_rows([first], c, 0, T, "fr")[0] for c in range(first.k)]
            first.release()
            # route a's host part over a sample, checked against the device's cells
            hp = min(a.host_perms, perms)
            step = PERIOD if units[0]["mode"] == "rounds" else 1
            t0 = time.perf_counter()
            got = [host_trace(params, [cols[j][p * step] for j in range(T_W)]) for p in range(hp)]
            packed = [pack([g[-1][0] for g in got])] if step == 1 else [pack([s[j] for g in got for s in g]) for j in range(T_W)]
            host_ms = (time.perf_counter() - t0) * 1e3 * perms / hp
            for p in (0, hp // 2, hp - 1):
                for c in range(len(rows)):
                    cell = lambda r: int.from_bytes(rows[c][32 * r:32 * r + 32], "big")   # noqa: E731
                    if step == 1:
                        assert cell(p) == got[p][-1][0]
                    else:
                        assert [cell(p * step + rho) for rho in range(FULL + PARTIAL + 1)] == [s[c] for s in got[p]]
            del packed

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

            warm = device()                             # (also the warm-up)
            assert check or warm == route_b()
            device()
            td, tb = [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                tb.append(timed(route_b, a.reps))
            md, mb = median(td), median(tb)
            line = {"metric": "poseidon", "T_log2": lg, "case": name, "t": T_W, "full": FULL, "partial": PARTIAL, "perms": perms,
                    "n_out": 0 if check else len(rows), "poseidon_ms": round(md, 4), "route_a_ms": round(host_ms + mb, 2),
                    "route_a_host_ms_scaled": round(host_ms, 2), "route_a_host_perms_timed": hp, "route_b_ms": round(mb, 4),
                    "poseidon_over_route_a": round(md / (host_ms + mb), 5), "poseidon_over_route_b": round(md / mb, 3),
                    "poseidon_rounds_ms": [round(x, 4) for x in td], "route_b_rounds_ms": [round(x, 4) for x in tb],
                    "poseidon_stages_ms": stages(device), **ident}
            if check:                                   # route c: the row unit that commits; route b is its one committed column
                def route_c():
                    s, _ = eng.commit_poseidon([A], params, [row_unit])
                    s.release()

                route_c()
                tc = [timed(route_c, a.reps) for _ in range(a.rounds)]
                line.update(route_c_ms=round(median(tc), 4), poseidon_over_route_c=round(md / median(tc), 3))
            print(json.dumps(line), flush=True)
        E.release()
        A.release()
        eng.close()


if __name__ == "__main__":
    main()
