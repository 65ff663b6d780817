"""The four builders with blinding rows (kzg_rows_commit_*_zk) against their plain calls, interleaved on the same box in the
same session, for T in {2^12, 2^16, 2^20} with usable = T - 6.

The instance is the standard 13-row circuit of scripts/bench_quotient.py with one lookup of wire c in a shuffle of its values
(as scripts/bench_quotient_ext.py builds it).  Everything is committed once, outside the timing.  The _zk calls run over the
same resident rows with usable = T - 6 and a five-scalar tail: their closing values are not 1 and 0 (the circuit fills all T
rows), which costs nothing and changes no launch.

  grand_product   kzg_rows_commit_grand_product_zk   against kzg_rows_commit_grand_product      (k = 3)
  lookup_sum      kzg_rows_commit_lookup_sum_zk      against kzg_rows_commit_lookup_sum         (L = 1, w = 1)
  multiplicities  kzg_rows_commit_multiplicities_zk  against kzg_rows_commit_multiplicities     (L = 1, w = 1)
  quotient        kzg_rows_commit_quotient_zk over the 13 rows and an all-ones active column (14 distinct rows) against
                  kzg_rows_commit_quotient_ext over the 13 rows: the same pieces (checked), one more extended row and one
                  more product per point

What to expect: the masks and the tail are two launches of one wave each, so the first three ratios should be 1 within the
spread that the plain call's own rounds show (plain_rounds_ms); the quotient's ratio should follow (distinct rows + 2) /
(distinct rows + 1) = 16 / 15 in its NTT share (L_0 is extended too).  One JSON line per size and builder, stamped with the
library identity like bench.py's lines.

    python scripts/bench_blinding.py [--rounds 3] [--reps 5] [--sizes 12,16,20]"""
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
from scripts.bench_quotient import SHIFTS, TERMS, be, instance, median  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        usable = T - 6
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        wires, sels, sig = instance(T, 77 + lg)
        rnd = random.Random(99 + lg)
        table = list(wires[2])
        rnd.shuffle(table)
        first = {}
        for t, v in enumerate(table):
            first.setdefault(v, t)
        mult = [0] * T
        for v in wires[2]:
            mult[first[v]] += 1
        tail = [be(rnd.randrange(1 << 250)) for _ in range(T - usable - 1)]
        beta, gamma, alpha, theta, lbeta = be(0xBE7A + lg), be(0x6A44A), be(0xA1FA + lg), be(0x7E7A + lg), be(0xBE7B + lg)
        rb = lambda rows: [b"".join(be(v) for v in r) for r in rows]   # noqa: E731
        AB, C, Q, SG = (eng.commit_rows(0, rb(x)) for x in (wires[:2], wires[2:], sels, sig))
        TB, M = eng.commit_rows(0, rb([table])), eng.commit_rows(0, rb([mult]))
        ONES = eng.commit_rows(0, rb([[1] * T]))
        bs = [be(s) for s in SHIFTS]
        Z, closing = eng.commit_grand_product([AB, C], [SG], bs, beta, gamma)
        assert closing == be(1), "the permutation does not close"
        del wires, sels, sig, table, mult
        S13 = [AB, C, Q, SG, Z]
        bt = [(be(c), idx) for c, idx in TERMS]
        bp = {"wires": [0, 1, 2], "sigmas": [9, 10, 11], "z": 12, "shifts": bs, "beta": beta, "gamma": gamma, "alpha": alpha}

        def once(call):
            def run():
                rs = call()
                rs = rs[0] if isinstance(rs, tuple) else rs
                rs.release()
                return rs.commitments
            return run

        pairs = {
            "grand_product": (once(lambda: eng.commit_grand_product_zk([AB, C], [SG], bs, beta, gamma, usable, tail)),
                              once(lambda: eng.commit_grand_product([AB, C], [SG], bs, beta, gamma))),
            "lookup_sum": (once(lambda: eng.commit_lookup_sum_zk([C], [TB], M, 1, 1, theta, lbeta, usable, tail)),
                           once(lambda: eng.commit_lookup_sum([C], [TB], M, 1, 1, theta, lbeta))),
            "multiplicities": (once(lambda: eng.commit_multiplicities_zk([C], [TB], 1, 1, usable, tail)),
                               once(lambda: eng.commit_multiplicities([C], [TB], 1, 1))),
            "quotient": (once(lambda: eng.commit_quotient_zk(S13 + [ONES], bt, bp, None, 13, 2, 3)),
                         once(lambda: eng.commit_quotient_ext(S13, bt, bp, None, 2, 3))),
        }
        assert pairs["quotient"][0]() == pairs["quotient"][1](), "an all-ones active column changed the pieces"

        def timed(f):
            samples = []
            for _ in range(a.reps):
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
            st = dict(zip(_native.TIMING_NAMES, tms))
            msm = sum(v for n, v in st.items() if n not in ("ntt", "poly", "total", "decode", "collective"))
            return {"ntt_ms": round(st["ntt"], 4), "poly_ms": round(st["poly"], 4), "msm_ms": round(msm, 4),
                    "total_ms": round(st["total"], 4)}

        for name, (zk, plain) in pairs.items():
            for f in (zk, plain):   # warm-up: workspace, twiddles, constants
                f()
            ta, tb = [], []
            for _ in range(a.rounds):    # interleaved: both forms see the same clock and thermal state
                ta.append(timed(zk))
                tb.append(timed(plain))
            ma, mb = median(ta), median(tb)
            print(json.dumps({"metric": "blinding", "builder": name, "T_log2": lg, "usable": usable, "zk_ms": round(ma, 4),
                              "plain_ms": round(mb, 4), "zk_over_plain": round(ma / mb, 3),
                              "zk_rounds_ms": [round(x, 4) for x in ta], "plain_rounds_ms": [round(x, 4) for x in tb],
                              "zk_stages": stages(zk), "plain_stages": stages(plain), **ident}), flush=True)
        for x in S13 + [TB, M, ONES]:
            x.release()
        eng.close()


if __name__ == "__main__":
    main()
