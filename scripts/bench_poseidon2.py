"""The device-built Poseidon2 columns (worker_commit_poseidon2's engine call) against the calls they stand beside, interleaved
on the same box, for T in {2^16, 2^20} at t = 3 with (R_F, R_P) = (8, 56) and t = 8 with (8, 57) (seeded random constants) in
three shapes: a row unit with one output column; a rounds unit with P = 128 (t columns, T / 128 permutations); a check of one
expected column.  The t source columns are committed once, outside the timing.

  poseidon2  commit_poseidon2 over the resident set: t forward transforms, ONE launch, n_out inverse transforms, one MSM pass
  route c    commit_poseidon at the same t, R_F, R_P (a Cauchy matrix) in the same run: THE YARDSTICK, never the new code itself
  route b    commit_rows of the n_out precomputed rows alone, upload included (read back from the device set once, outside the
             timing)

One JSON line per point with the ratios and the profiled `poly` stage (it holds the kernel) of both calls.  The expectation
under test is the product count: R_F 3 t + R_P (3 + t) against R_F (3 t + t^2) + R_P (3 + t^2), 408 / 816 and 819 / 4523.

    python scripts/bench_poseidon2.py [--rounds 3] [--reps 3] [--sizes 16,20]"""
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
PERIOD = 128
INSTANCES = [(3, 8, 56), (8, 8, 57)]


def make_params(t, full, partial, seed):
    """(the Poseidon2 parameters, the Poseidon parameters of the same t, R_F, R_P)"""
    rnd = random.Random(seed)
    sc = lambda n: [rnd.randrange(R) for _ in range(n)]   # noqa: E731
    return ({"t": t, "full": full, "partial": partial, "rc_full": sc(t * full), "rc_partial": sc(partial), "diag": sc(t)},
            {"t": t, "full": full, "partial": partial, "rc": sc(t * (full + partial)),
             "mds": [pow(1 + i + t + j, R - 2, R) for i in range(t) for j in range(t)]})


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(f, reps):
    samples = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        samples.append(time.perf_counter() - t0)
    return median(samples) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample (the median is reported)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x905E2 + lg, 0xFACADE, lg, 0)

        def stages(f):
            eng._chk(lib.kzg_set_profiling(eng._h, 1))
            try:
                f()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                eng._chk(lib.kzg_get_timings(eng._h, tms, len(tms)))
            finally:
                eng._chk(lib.kzg_set_profiling(eng._h, 0))
            return {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v}

        for t, full, partial in INSTANCES:
            p2, p1 = make_params(t, full, partial, 0x905E1D2 + t)
            rnd = random.Random(1000 * lg + t)
            A = eng.commit_rows(0, [b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(T)) for _ in range(t)])
            ins = list(range(t))
            row_unit = {"mode": "row", "in": ins, "out": [0]}
            rounds_unit = {"mode": "rounds", "in": ins, "period": PERIOD}
            E2, _ = eng.commit_poseidon2([A], p2, [row_unit])       # the expected columns of the checks, resident
            E1, _ = eng.commit_poseidon([A], p1, [row_unit])
            prods2 = full * 3 * t + partial * (3 + t)
            prods1 = full * (3 * t + t * t) + partial * (3 + t * t)
            shapes = [("row 1 output", [row_unit], T, None), ("rounds P=128 t columns", [rounds_unit], T // PERIOD, None),
                      ("check 1 column", [dict(row_unit, expect=[t])], T, (E2, E1))]
            for name, units, perms, exp in shapes:
                def call(fn, par, extra):
                    def f():
                        s, st = fn([A] + extra, par, units)
                        assert st["perms"] == [perms] and st["mismatch"] == [0]
                        if s is not None:
                            s.release()
                    return f

                new = call(eng.commit_poseidon2, p2, [exp[0]] if exp else [])
                old = call(eng.commit_poseidon, p1, [exp[1]] if exp else [])
                if exp:
                    rows = [eng.read_rows([E2], 0, 0, T, "fr")[0]]
                else:
                    first = eng.commit_poseidon2([A], p2, units)[0]
                    rows = [eng.read_rows([first], c, 0, T, "fr")[0] for c in range(first.k)]
                    first.release()

                def route_b():
                    eng.commit_rows(0, rows).release()

                for f in (new, old, route_b, new, old):    # (the warm-up)
                    f()
                tn, tc, tb = [], [], []
                for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                    tn.append(timed(new, a.reps))
                    tc.append(timed(old, a.reps))
                    tb.append(timed(route_b, a.reps))
                mn, mc, mb = median(tn), median(tc), median(tb)
                sn, so = stages(new), stages(old)
                line = {"metric": "poseidon2", "T_log2": lg, "case": name, "t": t, "full": full, "partial": partial, "perms": perms,
                        "n_out": 0 if exp else len(rows), "poseidon2_ms": round(mn, 4), "route_c_poseidon_ms": round(mc, 4),
                        "route_b_ms": round(mb, 4), "poseidon2_over_route_c": round(mn / mc, 3),
                        "poseidon2_over_route_b": round(mn / mb, 3), "products_poseidon2": prods2, "products_poseidon": prods1,
                        "products_ratio": round(prods2 / prods1, 4), "poseidon2_rounds_ms": [round(x, 4) for x in tn],
                        "route_c_rounds_ms": [round(x, 4) for x in tc], "route_b_rounds_ms": [round(x, 4) for x in tb],
                        "poseidon2_stages_ms": sn, "poseidon_stages_ms": so}
                if sn.get("poly") and so.get("poly"):
                    line["poly_ratio"] = round(sn["poly"] / so["poly"], 4)
                    line["poseidon2_gproducts_per_s"] = round(perms * prods2 / sn["poly"] / 1e6, 1)
                    line["poseidon_gproducts_per_s"] = round(perms * prods1 / so["poly"] / 1e6, 1)
                line["identity"] = ident
                print(json.dumps(line), flush=True)
            for s in (E2, E1, A):
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
