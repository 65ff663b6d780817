#!/usr/bin/env python3
"""Opening round over committed row sets, timed on one GPU: SHPLONK against the GWC calls it replaces.

  shplonk  (a) kzg_rows_commit_shplonk (round A: h built and committed on the device), then the host's round-B scalars and
               kzg_rows_open_lincomb over the rows followed by h at the one point u.  One proof pair, 96 bytes, 2 pairings.
  gwc      (b) kzg_rows_open_lincomb of the same rows at the same m points, four points per call (ceil(m / 4) calls): one
               proof per point, 48 m bytes.  Its verifier folds the points with random weights into 2 pairings per call.

Shapes: plonk (k = 15, m = 2: every row at zeta, the accumulator also at zeta w -- two MSMs on either route, so no gain is
expected), rot (k = 12, m = 4, three point sets: a gate with next- and previous-row rotations and a lookup sum), m8 (k = 12,
m = 8).  3 interleaved rounds; the sets are committed and the h sets of round A released outside the timing; every answer is
checked by the verifier before it is timed.  One JSON line per (size, shape).

    python scripts/bench_shplonk.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes plonk,rot,m8]"""
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


def rows_of(T, k, seed):
    rnd = random.Random(seed)
    return [b"".join(rnd.getrandbits(254).to_bytes(32, "big") for _ in range(T)) for _ in range(k)]


def median(xs):
    return sorted(xs)[len(xs) // 2]


def be(v):
    return (v % R).to_bytes(32, "big")


def shape_of(name, T, rnd):
    """(set sizes, points, opened)"""
    w, zeta = _root_of_unity(T), rnd.randrange(1, R)
    if name == "plonk":
        return (3, 1, 5, 3, 3), [zeta, zeta * w % R], [list(range(15)), [3]]
    if name == "rot":      # rows 0-7 at zeta; 8-9 also at zeta w; 10-11 at zeta w^-1, zeta, zeta w, zeta w^2
        return (8, 4), [zeta, zeta * w % R, zeta * pow(w, -1, R) % R, zeta * w * w % R], \
            [list(range(12)), [8, 9, 10, 11], [10, 11], [10, 11]]
    if name == "m8":       # eight rotations; rows 0-5 at zeta, 6-9 at four points, 10-11 at all eight
        return (6, 6), [zeta * pow(w, p, R) % R for p in range(8)], \
            [list(range(12)), [6, 7, 8, 9, 10, 11], [6, 7, 8, 9, 10, 11], [6, 7, 8, 9, 10, 11]] + [[10, 11]] * 4
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--shapes", default="plonk,rot,m8")
    a = ap.parse_args()
    ident = identity()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        for shape in a.shapes.split(","):
            rnd = random.Random(100 * lg + len(shape))
            sizes, pts, opened = shape_of(shape, T, rnd)
            k, m = sum(sizes), len(pts)
            P = [be(x) for x in pts]
            C = [be(rnd.randrange(1, R)) for _ in range(k)]
            u = be(rnd.randrange(R))
            rows = rows_of(T, k, 100 * lg + k)
            sets, o = [], 0
            for s in sizes:
                sets.append(eng.commit_rows(0, rows[o:o + s]))
                o += s
            comms = [c for s in sets for c in s.commitments]
            # the GWC route's combinations: row j with its c_j at every point it is opened at
            gwc = [[C[j] if j in js else be(0) for j in range(k)] for js in opened]

            made = []   # the h sets of the timed calls, released outside the timing

            def shplonk():
                W, hs = eng.commit_shplonk(sets, P, opened, C)
                made.append(hs)
                return W, eng.open_shplonk_finish(sets, hs, P, opened, C, u)[1]

            def gwc_route():
                out = []
                for p0 in range(0, m, 4):
                    out.append(eng.open_rows_lincomb(sets, P[p0:p0 + 4], gwc[p0:p0 + 4]))
                return out

            evals = []
            for p0 in range(0, m, 4):
                evals += eng.eval_rows(sets, P[p0:p0 + 4], opened[p0:p0 + 4])
            W, pi = shplonk()
            made.pop().release()
            assert eng.verify_open_shplonk(0, comms, P, opened, C, evals, W, u, pi), "the SHPLONK proof does not verify"
            for p0, (V, Pf) in zip(range(0, m, 4), gwc_route()):
                assert eng.verify_open_lincomb(0, comms, P[p0:p0 + 4], gwc[p0:p0 + 4], V, Pf), "the GWC proofs do not verify"

            def timed(f):
                samples = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                    while made:
                        made.pop().release()
                return median(samples) * 1e3

            for f in (shplonk, gwc_route):   # warm-up: buffers
                f()
            made.pop().release()
            ta, tb = [], []
            for _ in range(a.rounds):      # interleaved: both routes see the same clock and thermal state
                ta.append(timed(shplonk))
                tb.append(timed(gwc_route))
            ma, mb = median(ta), median(tb)
            calls = (m + 3) // 4
            print(json.dumps({"metric": "shplonk_open", "T_log2": lg, "shape": shape, "k": k, "m": m,
                              "shplonk_ms": round(ma, 4), "gwc_ms": round(mb, 4), "gwc_over_shplonk": round(mb / ma, 3),
                              "shplonk_rounds_ms": [round(x, 4) for x in ta], "gwc_rounds_ms": [round(x, 4) for x in tb],
                              "proof_bytes": {"shplonk": 96, "gwc": 48 * m}, "verifier_pairings": {"shplonk": 2, "gwc": 2 * calls},
                              "checked": True, **ident}), flush=True)
            for s in sets:
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
