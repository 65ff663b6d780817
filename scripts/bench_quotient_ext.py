"""The quotient with the lookup part (kzg_rows_commit_quotient_ext) against the plain standard quotient
(kzg_rows_commit_quotient), interleaved on the same box in the same session, for T in {2^12, 2^16, 2^20}.

The shape is the standard 13-row circuit of scripts/bench_quotient.py plus one lookup, 16 rows in all: L = 1, w = 1, the
input is wire c, the table row is a shuffle of c's values, m is committed and S is built by kzg_rows_commit_lookup_sum,
E = 4, P = 3.  Everything is committed once, outside the timing; z and S are built on the device, their closing values must
be 1 and 0, and the device's shape check confirms the instance on every call.

  ext    kzg_rows_commit_quotient_ext over the 16 resident rows: gate, permutation and lookup in one call
  plain  kzg_rows_commit_quotient over the first 13 of them (the same gate and permutation, the same alpha)

What to read off the split: the lookup costs three more extensions and transforms (table, m, S; c and L_0 are there already)
and the extra products of the pointwise kernel -- NTT grows by 3 / 14, POLY by the kernel's share -- and the MSM does not
change (three pieces either way).  It is not a second pass over the data.  At sizes up to --check-max the pieces are also
computed here (tests/quotient_ext_ref.py) and the commitments compared.  One JSON line per size, stamped with the library
identity like bench.py's lines.

    python scripts/bench_quotient_ext.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--check-max 12]"""
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

# row order: a b | c | qL qR qO qM qC PI | sigma1 sigma2 sigma3 | z | table | m | S
LOOKUP_ROWS = {"inputs": [2], "table": [13], "mult": 14, "sum": 15, "width": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--check-max", type=int, default=12, help="largest log2 size whose pieces are recomputed here and compared")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
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
        perm = {"wires": [0, 1, 2], "sigmas": [9, 10, 11], "z": 12, "shifts": SHIFTS, "beta": 0xBE7A + lg, "gamma": 0x6A44A,
                "alpha": 0xA1FA + lg}
        lookup = dict(LOOKUP_ROWS, theta=0x7E7A + lg, beta=0xBE7B + lg, alpha=perm["alpha"])
        rb = lambda rows: [b"".join(be(v) for v in r) for r in rows]   # noqa: E731
        AB, C, Q, SG = (eng.commit_rows(0, rb(x)) for x in (wires[:2], wires[2:], sels, sig))
        TB, M = eng.commit_rows(0, rb([table])), eng.commit_rows(0, rb([mult]))
        Z, closing = eng.commit_grand_product([AB, C], [SG], [be(s) for s in SHIFTS], be(perm["beta"]), be(perm["gamma"]))
        assert closing == be(1), "the permutation does not close"
        SUM, closing = eng.commit_lookup_sum([C], [TB], M, 1, 1, be(lookup["theta"]), be(lookup["beta"]))
        assert closing == be(0), "the lookup sum does not close"
        S13 = [AB, C, Q, SG, Z]
        S16 = S13 + [TB, M, SUM]
        bt = [(be(c), idx) for c, idx in TERMS]
        bp = dict(perm, shifts=[be(s) for s in SHIFTS], beta=be(perm["beta"]), gamma=be(perm["gamma"]), alpha=be(perm["alpha"]))
        bl = dict(lookup, theta=be(lookup["theta"]), beta=be(lookup["beta"]), alpha=be(lookup["alpha"]))
        checked = lg <= a.check_max
        if checked:
            from oracle import cpu as oc
            from tests import grand_product_ref as gref, lookup_ref as lref, quotient_ext_ref as xref, quotient_ref as qref
            z, cl = gref.grand_product(wires, sig, SHIFTS, perm["beta"], perm["gamma"])
            s_ev, cl0 = lref.lookup_sum([wires[2]], [table], mult, 1, 1, lookup["theta"], lookup["beta"])
            assert cl == 1 and cl0 == 0
            rows = wires + sels + sig + [z, table, mult, s_ev]
            t, rem = xref.quotient([qref.coeffs_of(r) for r in rows], TERMS, perm, lookup, 2)
            assert not any(rem) and qref.degree(t) == 3 * T - 4
            srs = oc.srs_gen(be(0x5EED + lg), be(0xFACADE), lg, 0, 0)
            want = [oc.commit(srs, qref.row_bytes(p), False) for p in qref.pieces(t, T, 3)]
        del wires, sels, sig, table, mult

        def ext():
            ts = eng.commit_quotient_ext(S16, bt, bp, bl, 2, 3)
            ts.release()
            return ts.commitments

        def plain():
            ts = eng.commit_quotient(S13, bt, bp, 2, 3)
            ts.release()
            return ts.commitments

        got = ext()
        assert all(not c[0] & 0x40 for c in got), "a piece commitment is the point at infinity: the instance is degenerate"
        assert got != plain(), "the lookup part changed nothing"
        if checked:
            assert got == want, "device quotient pieces != the oracle's commitments of the reference pieces"

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

        for f in (ext, plain):   # warm-up: workspace, twiddles, constants
            f()
        ta, tb = [], []
        for _ in range(a.rounds):    # interleaved: both forms see the same clock and thermal state
            ta.append(timed(ext))
            tb.append(timed(plain))
        ma, mb = median(ta), median(tb)
        print(json.dumps({"metric": "quotient_ext", "T_log2": lg, "rows": 16, "k": 3, "n_lookups": 1, "width": 1, "ext_log": 2,
                          "n_pieces": 3, "ext_ms": round(ma, 4), "plain_ms": round(mb, 4), "ext_over_plain": round(ma / mb, 3),
                          "ext_rounds_ms": [round(x, 4) for x in ta], "plain_rounds_ms": [round(x, 4) for x in tb],
                          "ext_stages": stages(ext), "plain_stages": stages(plain), "checked": checked, **ident}), flush=True)
        for x in S16:
            x.release()
        eng.close()


if __name__ == "__main__":
    main()
