"""The batched opening against k single-row calls: one kzg_commit_open_batch of k rows of a worker against k calls of
kzg_commit_open on the same host rows, interleaved on the same box, for T in {2^12, 2^16, 2^20} and k in {1, 2, 4, 8, 16}.
Before timing, the batched proof is checked against commit_open(i, h) for h = sum_j gamma^j f_j (and the commitments and
evaluations against the single calls'). One JSON line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_batch_open.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--ks 1,2,4,8,16]"""
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
from zkp_subnet_amd.engine import R_MODULUS as R  # noqa: E402


def rows_of(T, k, seed):
    rnd = random.Random(seed)
    return [b"".join(rnd.getrandbits(254).to_bytes(32, "big") for _ in range(T)) for _ in range(k)]


def combine(rows, gamma):
    T = len(rows[0]) // 32
    out = [0] * T
    for r in reversed(rows):
        out = [(a * gamma + int.from_bytes(r[32 * t:32 * t + 32], "big")) % R for t, a in enumerate(out)]
    return b"".join(v.to_bytes(32, "big") for v in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--ks", default="1,2,4,8,16")
    a = ap.parse_args()
    ident = identity()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        alpha = (0x1234567 + lg).to_bytes(32, "big")
        for k in [int(x) for x in a.ks.split(",")]:
            rows = rows_of(T, k, 100 * lg + k)
            gamma = random.Random(k).randrange(R)
            gb = gamma.to_bytes(32, "big")
            blob = b"".join(rows)   # the C-ABI's layout, prepared once: the host rows as kzg_commit_open_batch reads them
            C, Y, P = eng.commit_open_batch_joined(0, blob, k, alpha, gb)
            single = [eng.commit_open(0, r, alpha) for r in rows]
            assert C == [s[0] for s in single] and Y == [s[1] for s in single]
            assert P == eng.commit_open(0, combine(rows, gamma), alpha)[2], "batched proof != commit_open(i, h)"

            def batched():
                eng.commit_open_batch_joined(0, blob, k, alpha, gb)

            def separate():
                for r in rows:
                    eng.commit_open(0, r, alpha)

            for f in (batched, separate):   # warm-up: buffers and twiddles
                f()
            tb, ts = [], []
            for _ in range(a.rounds):      # interleaved: both forms see the same clock and thermal state
                for f, acc in ((batched, tb), (separate, ts)):
                    samples = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        f()
                        samples.append(time.perf_counter() - t0)
                    acc.append(sorted(samples)[len(samples) // 2] * 1e3)
            mb, ms_ = sorted(tb)[len(tb) // 2], sorted(ts)[len(ts) // 2]
            print(json.dumps({"metric": "batch_open", "T_log2": lg, "k": k, "batched_ms": round(mb, 4),
                              "separate_ms": round(ms_, 4), "speedup": round(ms_ / mb, 3),
                              "batched_rounds_ms": [round(x, 4) for x in tb], "separate_rounds_ms": [round(x, 4) for x in ts],
                              "proof_checked": True, **ident}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
