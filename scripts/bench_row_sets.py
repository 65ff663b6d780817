"""Committed row sets against today's sound route and the single-call lower bound, interleaved on the same box, for T in
{2^12, 2^16, 2^20} and the shapes of scripts/bench_multi_open.py: PLONK (k = 8, m = 2: every row at zeta, the last row also
at zeta * omega) and k = 4, m = 4 with full masks.

  sound    what a Fiat-Shamir caller does today: the commitments alone (the faster of k kzg_commit calls and one
           kzg_commit_open_batch at a throwaway point), then kzg_commit_open_multi (which uploads, transforms and commits
           every row again)
  sets     kzg_rows_commit, then kzg_rows_open, then kzg_rows_release
  single   one kzg_commit_open_multi: unsound under Fiat-Shamir (the points exist before the commitments), the lower
           bound the split route approaches

Before timing, the set route's commitments, evaluations and proofs are checked against kzg_commit_open_multi's.  One JSON
line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_row_sets.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes plonk,full4]"""
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


def median(xs):
    return sorted(xs)[len(xs) // 2]


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
            throwaway, one = (1).to_bytes(32, "big"), (1).to_bytes(32, "big")
            rows = rows_of(T, k, 100 * lg + k)
            blob = b"".join(rows)   # the C-ABI's layout, prepared once
            C, Y, Pf = eng.commit_open_multi_joined(0, blob, k, P, opened, G)
            with eng._commit_rows(0, k, blob, T, True) as rs:
                assert rs.commitments == C, "kzg_rows_commit != kzg_commit_open_multi commitments"
                assert eng.open_rows([rs], P, opened, G) == (Y, Pf), "kzg_rows_open != kzg_commit_open_multi"
            assert [eng.commit(0, r) for r in rows] == C

            def commits_single():
                for r in rows:
                    eng.commit(0, r)

            def commits_batch():
                eng.commit_open_batch_joined(0, blob, k, throwaway, one)

            def sets():
                rs = eng._commit_rows(0, k, blob, T, True)
                eng.open_rows([rs], P, opened, G)
                rs.release()

            def single():
                eng.commit_open_multi_joined(0, blob, k, P, opened, G)

            def timed(f):
                samples = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                return median(samples) * 1e3

            for f in (commits_single, commits_batch, sets, single):   # warm-up: buffers, twiddles, the set free list
                f()
            tcs, tcb, ts, t1 = [], [], [], []
            for _ in range(a.rounds):      # interleaved: every form sees the same clock and thermal state
                tcs.append(timed(commits_single))
                tcb.append(timed(commits_batch))
                ts.append(timed(sets))
                t1.append(timed(single))
            # today's sound route = the faster commitments-only form + one kzg_commit_open_multi
            commit_ms = min(median(tcs), median(tcb))
            sound = commit_ms + median(t1)
            ms, m1 = median(ts), median(t1)
            print(json.dumps({"metric": "row_sets", "T_log2": lg, "shape": shape, "k": k, "m": m,
                              "sets_ms": round(ms, 4), "sound_ms": round(sound, 4), "single_ms": round(m1, 4),
                              "speedup_vs_sound": round(sound / ms, 3), "over_single": round(ms / m1, 3),
                              "sound_commits": "kzg_commit x k" if median(tcs) <= median(tcb) else "commit_open_batch",
                              "commits_single_ms": round(median(tcs), 4), "commits_batch_ms": round(median(tcb), 4),
                              "sets_rounds_ms": [round(x, 4) for x in ts], "single_rounds_ms": [round(x, 4) for x in t1],
                              "checked": True, **ident}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
