"""Evaluate-then-open on committed row sets against today's sound route and the single-call lower bound, interleaved on the
same box, for T in {2^12, 2^16, 2^20}.  The sets are committed once, outside the timing: every route below starts from them.

  lincomb  (a) kzg_rows_eval, then kzg_rows_open_lincomb: the Fiat-Shamir order (the evaluations exist before the scalars)
  twice    (b) today's sound route: kzg_rows_open with throwaway gammas for the evaluations, then kzg_rows_open again
  single   (c) one kzg_rows_open: unsound under Fiat-Shamir (the gammas exist before the evaluations), the lower bound

Shapes:
  plonk  PLONK round 5: k = 15 rows in 5 sets (wires a, b, c | accumulator Z | five selectors | sigma1..3 | three quotient
         pieces); zeta opens ONE combination over all 15 rows (the linearisation's 10 rows plus v-weighted a, b, c, sigma1,
         sigma2), zeta * omega opens Z.  Routes (b) and (c) open the same polynomials the only way kzg_rows_open can: the
         five rows and the linearisation's 10 rows at zeta with gamma powers (the linearisation polynomial is not a set).
  full4  k = 4 rows in one set, m = 4 points with full masks.

Before timing, (a)'s proofs are checked against (b)/(c) where they prove the same combination (full4 with gamma powers) and
its evaluations against kzg_rows_open's.  One JSON line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_lincomb_open.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes plonk,full4]"""
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


def gamma_coeffs(k, opened, gammas):
    out = []
    for js, g in zip(opened, gammas):
        lam = [0] * k
        for t, j in enumerate(js):
            lam[j] = pow(int.from_bytes(g, "big"), t, R)
        out.append([be(x) for x in lam])
    return out


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
            rnd = random.Random(100 * lg + len(shape))
            zeta = rnd.randrange(R)
            if shape == "plonk":
                sizes = (3, 1, 5, 3, 3)   # a b c | Z | qL qR qO qM qC | s1 s2 s3 | t_lo t_mid t_hi
                k = 15
                P = [be(zeta), be(zeta * _root_of_unity(T))]
                lin = [4, 5, 6, 7, 8, 3, 11, 12, 13, 14]           # the linearisation's rows: selectors, Z, s3, t pieces
                five = [0, 1, 2, 9, 10]                            # a, b, c, s1, s2
                eval_opened = [five, [3]]
                lam0 = [0] * k
                for j in lin:
                    lam0[j] = rnd.randrange(R)
                v = rnd.randrange(R)
                for t, j in enumerate(five):
                    lam0[j] = pow(v, t + 1, R)
                lam1 = [0] * k
                lam1[3] = 1
                coeffs = [[be(x) for x in lam0], [be(x) for x in lam1]]
                open_opened = [sorted(five + lin), [3]]
            else:
                sizes, k = (4,), 4
                P = [be(rnd.randrange(R)) for _ in range(4)]
                eval_opened = open_opened = [list(range(k))] * 4
                coeffs = None
            m = len(P)
            G = [be(rnd.randrange(R)) for _ in range(m)]
            throwaway = [be(1)] * m
            if coeffs is None:
                coeffs = gamma_coeffs(k, open_opened, G)
            rows = rows_of(T, k, 100 * lg + k)
            sets, o = [], 0
            for s in sizes:
                sets.append(eng.commit_rows(0, rows[o:o + s]))
                o += s
            Y = eng.eval_rows(sets, P, eval_opened)
            Yo, Po = eng.open_rows(sets, P, open_opened, G)
            if shape == "plonk":   # zeta opens all 15 rows in (b) / (c): the five evaluations are among them
                assert Y == [[Yo[0][open_opened[0].index(j)] for j in five], Yo[1]], "kzg_rows_eval != kzg_rows_open"
            else:
                assert Y == Yo, "kzg_rows_eval != kzg_rows_open evaluations"
                assert eng.open_rows_lincomb(sets, P, coeffs)[1] == Po, "kzg_rows_open_lincomb != kzg_rows_open proofs"
            V, Pl = eng.open_rows_lincomb(sets, P, coeffs)
            assert eng.verify_open_lincomb(0, [c for s in sets for c in s.commitments], P, coeffs, V, Pl)

            def lincomb():
                eng.eval_rows(sets, P, eval_opened)
                eng.open_rows_lincomb(sets, P, coeffs)

            def twice():
                eng.open_rows(sets, P, open_opened, throwaway)
                eng.open_rows(sets, P, open_opened, G)

            def single():
                eng.open_rows(sets, P, open_opened, G)

            def timed(f):
                samples = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                return median(samples) * 1e3

            for f in (lincomb, twice, single):   # warm-up: buffers, twiddles
                f()
            ta, tb, tc = [], [], []
            for _ in range(a.rounds):      # interleaved: every form sees the same clock and thermal state
                ta.append(timed(lincomb))
                tb.append(timed(twice))
                tc.append(timed(single))
            ma, mb, mc = median(ta), median(tb), median(tc)
            print(json.dumps({"metric": "lincomb_open", "T_log2": lg, "shape": shape, "k": k, "m": m,
                              "lincomb_ms": round(ma, 4), "twice_ms": round(mb, 4), "single_ms": round(mc, 4),
                              "speedup_vs_twice": round(mb / ma, 3), "over_single": round(ma / mc, 3),
                              "lincomb_rounds_ms": [round(x, 4) for x in ta], "twice_rounds_ms": [round(x, 4) for x in tb],
                              "single_rounds_ms": [round(x, 4) for x in tc], "checked": True, **ident}), flush=True)
            for s in sets:
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
