"""The four calls with per-row lookup selectors (kzg_rows_commit_multiplicities_sel, kzg_rows_commit_lookup_sum_sel,
kzg_rows_commit_quotient_sel, kzg_rows_quotient_part_sel) against their existing siblings on the same resident rows, interleaved on the same box in the same session: L = 2 lookups of width
w = 2, T in {2^16, 2^20}, the plain layout (usable = T).

The instance: a table of T random 2-tuples, two 0/1 selector columns (about half the rows enabled), enabled cells drawn from
the table and disabled cells random (in no table row).  Everything is committed once, outside the timing.  Three forms per
builder over the SAME rows:
  plain     the existing call (it sees the disabled cells as misses / the sum does not close: the launches are what is timed)
  sentinel  the _sel call with every entry KZG_NO_SELECTOR: the existing call's launches behind the _sel entry point
  sel       the _sel call with the two distinct selector rows: two more forward transforms, the selector probe / LK_INPUT_SEL
The quotient forms run the lookup relation alone over the ten rows inputs | table | q_0 q_1 | m | S at ext_log = 2 with 4
pieces (plain: kzg_rows_commit_quotient_zk / kzg_rows_quotient_part, whose relation does not hold on these rows -- with P = E
pieces nothing is checked and the launches are the same; sel: two more extended rows, k_quot_points_sel).
What is reported is sel_over_plain, the selector's marginal cost; no ratio is asserted.  One JSON line per size and builder,
stamped with the library identity like bench.py's lines.

    python scripts/bench_lookup_selectors.py [--rounds 3] [--reps 5] [--sizes 16,20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from zkp_subnet_amd import HipEngine  # noqa: E402

L, W = 2, 2


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def be(v):
    return int(v).to_bytes(32, "big")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        rng = np.random.default_rng(0x5E1 + lg)
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)

        def rand_col():   # T scalars below 2^248 as 32 big-endian bytes each
            col = rng.integers(0, 256, size=(T, 32), dtype=np.uint8)
            col[:, 0] = 0
            return col

        table = [rand_col() for _ in range(W)]
        inputs, sels = [], []
        for _ in range(L):
            on = rng.integers(0, 2, size=T, dtype=np.uint8)
            pick = rng.integers(0, T, size=T)
            q = np.zeros((T, 32), dtype=np.uint8)
            q[:, 31] = on
            sels.append(q)
            for c in range(W):
                inputs.append(np.where(on[:, None] == 1, table[c][pick], rand_col()))
        rb = lambda cols: [c.tobytes() for c in cols]   # noqa: E731
        F, TB, Q = eng.commit_rows(0, rb(inputs)), eng.commit_rows(0, rb(table)), eng.commit_rows(0, rb(sels))
        enabled = int(sum(int(q[:, 31].sum()) for q in sels))
        del table, inputs, sels
        theta, beta = be(0x7E7A + lg), be(0xBE7B + lg)
        M, missing = eng.commit_multiplicities_sel([F], [TB], [Q], [0, 1], L, W)
        assert missing == 0, "an enabled cell is in no table row"
        S, closing = eng.commit_lookup_sum_sel([F], [TB], M, [Q], [0, 1], L, W, theta, beta)
        assert closing == be(0), "the sum with selectors does not close"
        rows = [F, TB, Q, M, S]   # inputs 0 - 3, table 4 5, selectors 6 7, m 8, S 9
        lk = {"inputs": [0, 1, 2, 3], "table": [4, 5], "mult": 8, "sum": 9, "width": W, "theta": theta, "beta": beta,
              "alpha": be(0xA1FA + lg)}
        eng.commit_quotient_sel(rows, [], None, lk, [6, 7], None, 2, 3).release()   # the relation holds: t fits 3 pieces

        def once(call):
            def run():
                rs = call()
                rs = rs[0] if isinstance(rs, tuple) else rs
                rs.release()
                return getattr(rs, "commitments", None)
            return run

        forms = {
            "multiplicities": {
                "plain": once(lambda: eng.commit_multiplicities([F], [TB], L, W)),
                "sentinel": once(lambda: eng.commit_multiplicities_sel([F], [TB], [], [None, None], L, W)),
                "sel": once(lambda: eng.commit_multiplicities_sel([F], [TB], [Q], [0, 1], L, W))},
            "lookup_sum": {
                "plain": once(lambda: eng.commit_lookup_sum([F], [TB], M, L, W, theta, beta)),
                "sentinel": once(lambda: eng.commit_lookup_sum_sel([F], [TB], M, [], [None, None], L, W, theta, beta)),
                "sel": once(lambda: eng.commit_lookup_sum_sel([F], [TB], M, [Q], [0, 1], L, W, theta, beta))},
            "quotient": {
                "plain": once(lambda: eng.commit_quotient_zk(rows, [], None, lk, None, 2, 4)),
                "sentinel": once(lambda: eng.commit_quotient_sel(rows, [], None, lk, [None, None], None, 2, 4)),
                "sel": once(lambda: eng.commit_quotient_sel(rows, [], None, lk, [6, 7], None, 2, 4))},
            "quotient_part": {
                "plain": once(lambda: eng.quotient_part(rows, [], None, lk, None, None, 2)),
                "sentinel": once(lambda: eng.quotient_part_sel(rows, [], None, lk, [None, None], None, None, 2)),
                "sel": once(lambda: eng.quotient_part_sel(rows, [], None, lk, [6, 7], None, None, 2))},
        }

        def timed(f):
            samples = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f()
                samples.append(time.perf_counter() - t0)
            return median(samples) * 1e3

        for name, fs in forms.items():
            assert fs["plain"]() == fs["sentinel"](), "the sentinel call is not the existing call"
            fs["sel"]()   # warm-up: workspace, twiddles
            rounds = {k: [] for k in fs}
            for _ in range(a.rounds):    # interleaved: the three forms see the same clock and thermal state
                for k, f in fs.items():
                    rounds[k].append(timed(f))
            med = {k: median(v) for k, v in rounds.items()}
            print(json.dumps({"metric": "lookup_selectors", "builder": name, "T_log2": lg, "L": L, "w": W, "enabled_cells": enabled,
                              **{k + "_ms": round(v, 4) for k, v in med.items()},
                              "sel_over_plain": round(med["sel"] / med["plain"], 3),
                              "sentinel_over_plain": round(med["sentinel"] / med["plain"], 3),
                              **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in rounds.items()}, **ident}), flush=True)
        for x in (F, TB, Q, M, S):
            x.release()
        eng.close()


if __name__ == "__main__":
    main()
