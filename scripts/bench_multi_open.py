"""The multi-point opening against composing today's calls: one kzg_commit_open_multi of k rows of a worker at m points
against one kzg_commit_open_batch per point over that point's rows, interleaved on the same box, for T in {2^12, 2^16,
2^20} and two shapes: PLONK (k = 8, m = 2: every row at zeta, the last row also at zeta * omega) and k = 4, m = 4 with
full masks.  Before timing, the multi-point call's outputs are checked against the composed calls' (commitments,
evaluations, proofs).  One JSON line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_multi_open.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes plonk,full4]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from zkp_subnet_amd import HipEngine  # noqa: E402
from zkp_subnet_amd.engine import R_MODULUS as R, _root_of_unity  # noqa: E402

SHAPES = {"plonk": (8, lambda k: [list(range(k)), [k - 1]]), "full4": (4, lambda k: [list(range(k))] * 4)}


def rows_of(T, k, seed):
    rnd = random.Random(seed)
    return [b"".join(rnd.getrandbits(254).to_bytes(32, "big") for _ in range(T)) for _ in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--shapes", default="plonk,full4")
    a = ap.parse_args()
    ident = identity()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        for shape in a.shapes.split(","):
            k, opened_of = SHAPES[shape]
            opened = opened_of(k)
            m = len(opened)
            rnd = random.Random(100 * lg + k)
            zeta = rnd.randrange(R)
            pts = [zeta, zeta * _root_of_unity(T) % R] + [rnd.randrange(R) for _ in range(m - 2)]
            P = [x.to_bytes(32, "big") for x in pts]
            G = [rnd.randrange(R).to_bytes(32, "big") for _ in range(m)]
            rows = rows_of(T, k, 100 * lg + k)
            blob = b"".join(rows)   # the C-ABI's layout, prepared once
            subs = [(b"".join(rows[j] for j in js), len(js)) for js in opened]
            C, Y, Pf = eng.commit_open_multi_joined(0, blob, k, P, opened, G)
            for p, (js, (sb, n)) in enumerate(zip(opened, subs)):
                Cb, Yb, Pb = eng.commit_open_batch_joined(0, sb, n, P[p], G[p])
                assert Cb == [C[j] for j in js] and Yb == Y[p] and Pb == Pf[p], "multi-point call != composed batch calls"

            def multi():
                eng.commit_open_multi_joined(0, blob, k, P, opened, G)

            def composed():
                for p, (sb, n) in enumerate(subs):
                    eng.commit_open_batch_joined(0, sb, n, P[p], G[p])

            for f in (multi, composed):   # warm-up: buffers and twiddles
                f()
            tm, tc = [], []
            for _ in range(a.rounds):      # interleaved: both forms see the same clock and thermal state
                for f, acc in ((multi, tm), (composed, tc)):
                    samples = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        f()
                        samples.append(time.perf_counter() - t0)
                    acc.append(sorted(samples)[len(samples) // 2] * 1e3)
            mm, mc = sorted(tm)[len(tm) // 2], sorted(tc)[len(tc) // 2]
            print(json.dumps({"metric": "multi_open", "T_log2": lg, "shape": shape, "k": k, "m": m,
                              "multi_ms": round(mm, 4), "composed_ms": round(mc, 4), "speedup": round(mc / mm, 3),
                              "multi_rounds_ms": [round(x, 4) for x in tm], "composed_rounds_ms": [round(x, 4) for x in tc],
                              "checked": True, **ident}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
