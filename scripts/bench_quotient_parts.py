"""The quotient in parts (kzg_rows_quotient_part / _finish) against the single call, interleaved on the same box in the same
session, for T in {2^12, 2^16, 2^20}.  Two shapes, everything committed once outside the timing:

  (a) overhead   the standard 13-row circuit of scripts/bench_quotient.py with an all-ones active column (14 rows, k = 3,
                 ext_log = 2, 3 pieces): ONE kzg_rows_commit_quotient_zk call against THREE parts (the gate terms in two halves,
                 the permutation) + finish.  What the mechanism costs when it is not needed: the wires are extended three times
                 instead of once, and three adds.  The pieces are the same bytes (checked).
  (b) chunks     a 6-wire circuit with one selector that still fits 16 rows (6 wires, 6 sigmas, q, A, z: 15): today's only
                 route, one call at ext_log = 3 (k = 6 <= E - 1 = 7; 8 pieces), against two chunks of 3 wires at ext_log = 2
                 (their z_c chained on the device, 4 pieces) through three parts + finish.  The identity permutation and a zero
                 selector: the work does not depend on the values.

One JSON line per size and shape with the NTT / POLY / MSM split of each side, stamped with the library identity like
bench.py's lines.

    python scripts/bench_quotient_parts.py [--rounds 3] [--reps 5] [--sizes 12,16,20]"""
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
from zkp_subnet_amd.engine import R_MODULUS as R  # noqa: E402


def omega(T):
    """the library's T-th root of unity: 7^((r-1)/T)"""
    return pow(7, (R - 1) // T, R)


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
        rnd = random.Random(199 + lg)
        rb = lambda rows: [b"".join(be(v) for v in r) for r in rows]   # noqa: E731
        tail = [be(rnd.randrange(1 << 250)) for _ in range(T - usable - 1)]
        beta, gamma, alpha = be(0xBE7A + lg), be(0x6A44A), be(0xA1FA + lg)
        # ---- (a) the 13-row circuit + A
        wires, sels, sig = instance(T, 77 + lg)
        AB, C, Q, SG = (eng.commit_rows(0, rb(x)) for x in (wires[:2], wires[2:], sels, sig))
        ONES = eng.commit_rows(0, rb([[1] * T]))
        bs = [be(s) for s in SHIFTS]
        Z, closing = eng.commit_grand_product([AB, C], [SG], bs, beta, gamma)
        assert closing == be(1), "the permutation does not close"
        del wires, sels, sig
        S14 = [AB, C, Q, SG, Z, ONES]
        bt = [(be(c), idx) for c, idx in TERMS]
        bp = {"wires": [0, 1, 2], "sigmas": [9, 10, 11], "z": 12, "shifts": bs, "beta": beta, "gamma": gamma, "alpha": alpha}
        half = len(bt) // 2
        pp = {"wires": [0, 1, 2], "sigmas": [3, 4, 5], "z": 6, "shifts": bs, "beta": beta, "gamma": gamma, "alpha": alpha}

        def single_a():
            rs = eng.commit_quotient_zk(S14, bt, bp, None, 13, 2, 3)
            rs.release()
            return rs.commitments

        def parts_a():
            acc = eng.quotient_part([AB, C, Q], bt[:half], None, None, None, None, 2, None)
            eng.quotient_part([AB, C, Q], bt[half:], None, None, None, None, 2, None, acc)
            eng.quotient_part([AB, C, SG, Z, ONES], [], pp, None, 7, None, 2, None, acc)
            rs = eng.quotient_finish(acc, 3)
            rs.release()
            return rs.commitments

        assert single_a() == parts_a(), "three parts changed the pieces"
        # ---- (b) six wires, one selector
        w6 = [[rnd.randrange(R) for _ in range(T)] for _ in range(6)]
        om, dom = omega(T), [1] * T
        for t in range(1, T):
            dom[t] = dom[t - 1] * om % R
        sh6 = [pow(7, j, R) for j in range(6)]
        W6 = [eng.commit_rows(0, rb([r])) for r in w6]
        G6 = [eng.commit_rows(0, rb([[s * x % R for x in dom]])) for s in sh6]
        QZ = eng.commit_rows(0, rb([[0] * T]))
        ACT = eng.commit_rows(0, rb([[1] * usable + [0] * (T - usable)]))
        del w6, dom
        b6 = [be(s) for s in sh6]
        Z6, c6 = eng.commit_grand_product_zk(W6, G6, b6, beta, gamma, usable, tail)
        Z0, c0 = eng.commit_grand_product_chain(W6[:3], G6[:3], b6[:3], beta, gamma, usable, tail, be(1))
        Z1, c1 = eng.commit_grand_product_chain(W6[3:], G6[3:], b6[3:], beta, gamma, usable, tail, c0)
        assert c6 == c1 == be(1), "the identity permutation does not close"
        gate6 = [(be(1), [6, 0, 1]), (be(1), [6, 2]), (be(1), [6, 3, 4]), (be(1), [6, 5])]
        p6 = {"wires": list(range(6)), "sigmas": list(range(7, 13)), "z": 14, "shifts": b6, "beta": beta, "gamma": gamma,
              "alpha": alpha}
        pc = [{"wires": [0, 1, 2], "sigmas": [3, 4, 5], "z": 7, "shifts": b6[3 * c:3 * c + 3], "beta": beta, "gamma": gamma,
               "alpha": alpha} for c in range(2)]

        def single_b():
            rs = eng.commit_quotient_zk(W6 + [QZ] + G6 + [ACT, Z6], gate6, p6, None, 13, 3, 8)
            rs.release()
            return rs.commitments

        def parts_b():
            acc = eng.quotient_part(W6 + [QZ], gate6, None, None, None, None, 2, None)
            eng.quotient_part(W6[:3] + G6[:3] + [ACT, Z0], [], pc[0], None, 6, None, 2, alpha, acc)
            eng.quotient_part(W6[3:] + G6[3:] + [ACT, Z1, Z0], [], pc[1], None, 6, (8, usable), 2, beta, acc)
            rs = eng.quotient_finish(acc, 4)
            rs.release()
            return rs.commitments

        def timed(f):
            samples = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f()
                samples.append(time.perf_counter() - t0)
            return median(samples) * 1e3

        def stages(f):
            """the NTT / POLY / MSM split, summed over the calls f makes (the library keeps the last call's stage times)"""
            eng._chk(lib.kzg_set_profiling(eng._h, 1))
            tot, last = {}, [None]
            orig = eng._chk

            def chk(rc):
                orig(rc)
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                orig(lib.kzg_get_timings(eng._h, tms, len(tms)))
                if tuple(tms) == last[0]:      # a call that runs no kernel (a release) leaves the last call's times
                    return
                last[0] = tuple(tms)
                for n, v in zip(_native.TIMING_NAMES, tms):
                    tot[n] = tot.get(n, 0.0) + v
            eng._chk = chk
            try:
                f()
            finally:
                eng._chk = orig
                eng._chk(lib.kzg_set_profiling(eng._h, 0))
            msm = sum(v for n, v in tot.items() if n not in ("ntt", "poly", "total", "decode", "collective"))
            return {"ntt_ms": round(tot.get("ntt", 0), 4), "poly_ms": round(tot.get("poly", 0), 4), "msm_ms": round(msm, 4),
                    "total_ms": round(tot.get("total", 0), 4)}

        for name, single, parts in (("overhead_14_rows", single_a, parts_a), ("six_wires_E8_vs_two_chunks_E4", single_b, parts_b)):
            for f in (single, parts):   # warm-up: workspace, twiddles, constants
                f()
            ta, tb = [], []
            for _ in range(a.rounds):    # interleaved: both routes see the same clock and thermal state
                ta.append(timed(parts))
                tb.append(timed(single))
            ma, mb = median(ta), median(tb)
            print(json.dumps({"metric": "quotient_parts", "shape": name, "T_log2": lg, "usable": usable, "parts_ms": round(ma, 4),
                              "single_ms": round(mb, 4), "parts_over_single": round(ma / mb, 3),
                              "parts_rounds_ms": [round(x, 4) for x in ta], "single_rounds_ms": [round(x, 4) for x in tb],
                              "parts_stages": stages(parts), "single_stages": stages(single), **ident}), flush=True)
        for x in S14 + W6 + G6 + [QZ, ACT, Z6, Z0, Z1]:
            x.release()
        eng.close()


if __name__ == "__main__":
    main()
