"""CPU-only tests of the quotient in parts and the chained grand product (kzg_rows_quotient_part / _finish,
kzg_rows_commit_grand_product_chain, the text forms on Client and MultiDeviceClient): the reference
(tests/quotient_parts_ref.py) pinned against the single call's reference, what a wide instance's numerator says about satisfied
and broken instances, the preconditions of every instance the GPU tests use, header / ctypes agreement, and the host logic over
a fake engine defined here."""
import hashlib
import itertools
import os
import re

import pytest

from tests import blinding_ref as br
from tests import quotient_parts_ref as qp
from tests import quotient_ref as qr
from tests.quotient_parts_ref import GPU_CLIENT, GPU_SPLIT, GPU_WIDE
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr
from zkp_subnet_amd.engine import QuotientAcc, RowSet

R = qp.R
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def split_three(inst):
    """blinding_ref.Instance as three parts -- gate, permutation, lookup -- each over its own rows and numbering"""
    rows = inst.coeff_rows()
    gate_names = [br.A_, br.B_, br.C_, br.QM, br.QL, br.QC, br.ACT, br.LU, br.Z_, br.SUM]
    g = {n: j for j, n in enumerate(gate_names)}
    gate = qp.part([rows[n] for n in gate_names], [(c, [g[f] for f in fs]) for c, fs in inst.terms])
    pn = [br.A_, br.B_, br.C_, br.S1, br.S2, br.S3, br.Z_, br.ACT]
    perm = dict(inst.perm, wires=[0, 1, 2], sigmas=[3, 4, 5], z=6)
    ln = [br.C_, br.TAB, br.M_, br.SUM, br.ACT]
    lookup = dict(inst.lookup, inputs=[0], table=[1], mult=2, sum=3)
    return [gate, qp.part([rows[n] for n in pn], [], perm, None, 7), qp.part([rows[n] for n in ln], [], None, lookup, 4)]


# ---------------------------------------------------------------------------------------------------- the reference
def test_three_parts_sum_to_the_one_call_numerator():
    inst = br.Instance(16, 11, 31)
    one = br.numerator(inst.coeff_rows(), inst.terms, inst.perm, inst.lookup, inst.active, 3)
    parts = split_three(inst)
    assert qr.trim(qp.numerator(parts, 3)) == qr.trim(one)
    # ... and a scale weighs its part alone
    parts[1]["scale"] = 5
    assert qr.trim(qp.numerator(parts, 3)) == qr.trim(qr.add(one, qr.scale(qp.part_numerator(parts[1], 3), 4)))


def test_the_linked_p2_is_z_minus_the_rotated_row_times_l0():
    T, rot = 8, 3
    rows = [qr.coeffs_of([(7 * t + j) % R for t in range(T)]) for j in range(6)] + [qr.coeffs_of([1] * T)]
    perm = {"wires": [0], "sigmas": [1], "z": 2, "shifts": [1], "beta": 3, "gamma": 5, "alpha": 11}
    linked = qp.part_numerator(qp.part(rows, [], perm, None, 6, (4, rot)), 2)
    plain = qp.part_numerator(qp.part(rows, [], perm, None, 6), 2)
    # the difference is alpha^2 (1 - f_4(w^rot X)) L_0(X): on the domain, (1 - f_4(w^rot)) at row 0 and 0 elsewhere
    diff = qr.sub(linked, plain)
    ev = [qr.poly_eval(diff, x) for x in qp.gp.domain(T)]
    f4 = qr.evals_of(rows[4])
    assert ev == [121 * (1 - f4[rot]) % R] + [0] * (T - 1)


def test_grand_product_chain_scales_rows_up_to_usable():
    T, u = 16, 11
    w = qp.WideInstance(T, u, 3)
    z, cl = br.grand_product_zk(w.wires[:3], w.sig[:3], w.shifts[:3], w.beta, w.gamma, u, w.tails[0])
    zc, clc = qp.grand_product_chain(w.wires[:3], w.sig[:3], w.shifts[:3], w.beta, w.gamma, u, w.tails[0], 9)
    assert zc[:u + 1] == [9 * v % R for v in z[:u + 1]] and zc[u + 1:] == z[u + 1:] == w.tails[0] and clc == 9 * cl % R
    assert qp.grand_product_chain(w.wires[:3], w.sig[:3], w.shifts[:3], w.beta, w.gamma, u, w.tails[0], 1) == (z, cl)


def test_wide_instance_divides_and_each_broken_one_does_not():
    T, u = 16, 11
    w = qp.WideInstance(T, u, 5)
    assert w.closing0 not in (0, 1) and w.closing1 == 1 and w.denominators_nonzero()
    assert len({id(r) for r in w.all_rows}) == qp.NAMES > 16
    assert all(len(p["rows"]) <= 16 for p in w.parts())
    t, rem = qp.quotient(w.parts(), 2)
    assert not any(rem)
    # A P1 has k + 2 = 5 factors of degree T - 1: deg t <= 4 T - 5, so t fits E = 4 pieces (not fewer, for a random instance)
    assert 3 * T < len(t) <= 4 * T - 4
    val_rows = w.parts()
    x = 0x1234567
    vals = [(p, (lambda p: lambda j, rot: qr.poly_eval(p["rows"][j], pow(qp.gp.omega(T), rot % T, R) * x % R))(p)) for p in val_rows]
    assert qp.num_at(vals, x, T) == qr.poly_eval(t, x) * (pow(x, T, R) - 1) % R
    for breaker in ("broken_cell", "broken_start", "broken_rot"):
        b = getattr(qp.WideInstance(T, u, 5), breaker)()
        assert b.denominators_nonzero()
        assert any(qp.quotient(b.parts(), 2)[1]), breaker


def test_preconditions_of_the_gpu_instances():
    for lg, u, seed in GPU_WIDE + [GPU_CLIENT]:
        w = qp.WideInstance(1 << lg, u, seed)
        assert w.denominators_nonzero() and w.closing0 not in (0, 1) and w.closing1 == 1
        for breaker in ("broken_cell", "broken_start", "broken_rot"):
            if lg > 8:
                continue
            b = getattr(qp.WideInstance(1 << lg, u, seed), breaker)()
            assert b.denominators_nonzero() and b.closing0 != 0 and b.closing1 != 0
    for lg, u, seed in GPU_SPLIT:
        inst = br.Instance(1 << lg, u, seed)
        _, D = qp.gp.factors(inst.wires, [inst.fixed[j] for j in (br.S1, br.S2, br.S3)], inst.shifts, inst.beta, inst.gamma)
        assert all(D[:u]) and inst.z_closing == 1 and inst.S_closing == 0 and inst.missing == 0


# ---------------------------------------------------------------------------------------------------- the C-ABI's surface
def test_header_bindings_and_docs_agree():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_quotient_part", "kzg_rows_quotient_finish", "kzg_rows_commit_grand_product_chain"):
        for pre in ("", "kzg_multi_"):
            sym = pre + name[4:] if pre else name
            m = re.search(r"\nint " + sym + r"\(([^;]*)\);", hdr)
            assert m, sym
            params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
            assert len(params.split(",")) == len(_native.SYMBOLS[sym][1]), sym
    assert "typedef struct kzg_quotient_link" in hdr
    assert [f[0] for f in _native.QuotientLink._fields_] == ["prev_row", "rot"]
    for word in ("OUT OF SCOPE", "transformed twice", "more than 16 rows", "plookup", "Degree-raising blinders".lower()):
        assert word in hdr, word


# ---------------------------------------------------------------------------------------------------- the text forms
class FakeEngine:
    """the accumulator semantics over stand-in arithmetic: a part's contribution is a hash of what it depends on"""

    def __init__(self):
        self.sets, self.accs, self.calls, self.workers = {}, {}, [], None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    def commit_rows(self, i, rows, evaluation_form=True):
        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32, [hashlib.sha384(b"C" + r).digest() for r in rows])

    def quotient_part(self, sets, terms, perm, lookup, active_row, link, ext_log, scale_be32, acc=None):
        hs = [int(x) for x in sets]
        self.calls.append(("part", tuple(hs), active_row, link, ext_log, scale_be32, acc.handle if acc else None))
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        i = self.sets[hs[0]][0]
        blob = hashlib.sha256(repr((hs, terms, perm, lookup, active_row, link, ext_log, scale_be32)).encode()).digest()
        if acc is None:
            acc = QuotientAcc(self, next(_HANDLES), i, len(self.sets[hs[0]][1][0]) // 32, ext_log)
            self.accs[acc.handle] = []
        elif acc.handle not in self.accs or acc.ext_log != ext_log or acc.i != i:
            raise _native.KzgError(E_ARG, "the part's worker, row length and ext_log must be the accumulator's")
        self.accs[acc.handle].append(blob)
        return acc

    def quotient_finish(self, acc, n_pieces):
        self.calls.append(("finish", acc.handle, n_pieces))
        blobs = self.accs.pop(acc.handle)
        h = next(_HANDLES)
        self.sets[h] = (acc.i, [b"\0" * 32 * acc.T] * n_pieces)
        return RowSet(self, h, acc.i, n_pieces, acc.T, [hashlib.sha384(b"T%d" % p + b"".join(sorted(blobs))).digest()
                                                        for p in range(n_pieces)])

    def commit_grand_product_chain(self, wire_sets, sigma_sets, shifts, beta, gamma, usable, tail, start):
        hs = [int(x) for x in list(wire_sets) + list(sigma_sets)]
        self.calls.append(("chain", tuple(hs), tuple(shifts), beta, gamma, usable, tuple(tail), start))
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        i, h = self.sets[hs[0]][0], next(_HANDLES)
        self.sets[h] = (i, [b"\0" * len(self.sets[hs[0]][1][0])])
        return RowSet(self, h, i, 1, len(self.sets[hs[0]][1][0]) // 32, [hashlib.sha384(b"Z" + start).digest()]), start

    def release_rows(self, handle):
        if self.sets.pop(int(handle), None) is None and self.accs.pop(int(handle), None) is None:
            raise _native.KzgError(E_ARG, "unknown or already released handle")


def fr(v):
    return be32_to_fr(v.to_bytes(32, "big"))


def polys(k, T, seed):
    return [[fr(seed * 1000 + j * 100 + t) for t in range(T)] for j in range(k)]


TERMS = [[fr(1), [0, [1, 1]]]]
PERM = {"wires": [0], "sigmas": [1], "z": 2, "shifts": [fr(1)], "beta": fr(3), "gamma": fr(5), "alpha": fr(7)}


def test_client_parts_over_a_fake_engine():
    eng = FakeEngine()
    cl = Client(engine=eng)
    cl.machines_scale, cl._slice_of = 2, None   # what start() leaves for a synthetic setup
    a = cl.worker_commit_rows(0, polys(3, 8, 1)).json()["handle"]
    r = cl.worker_quotient_part([a], TERMS, PERM, None, 2, [1, -1], 2, fr(9))
    assert r.status_code == 200, r.json()
    acc = r.json()["acc"]
    assert eng.calls[-1] == ("part", (a,), 2, (1, -1), 2, (9).to_bytes(32, "big"), None)
    r = cl.worker_quotient_part([a], TERMS, acc=acc)
    assert r.status_code == 200 and r.json()["acc"] == acc and eng.calls[-1][-2:] == (None, acc)
    # argument checks: a link without a permutation part, a scale >= r, a malformed link, an unknown accumulator
    assert cl.worker_quotient_part([a], TERMS, None, None, None, [1, 0]).status_code == 400
    assert cl.worker_quotient_part([a], TERMS, scale=be32_to_fr(R.to_bytes(32, "big"))).status_code == 400
    assert cl.worker_quotient_part([a], TERMS, PERM, None, None, [1]).status_code == 400
    assert cl.worker_quotient_part([a], TERMS, acc=10 ** 9).status_code == 400
    assert cl.worker_quotient_part([a], TERMS, acc=acc, ext_log=3).status_code == 400     # the engine's KZG_E_ARG
    assert cl.worker_quotient_finish(acc, 0).status_code == 400 and cl.worker_quotient_finish(acc, "x").status_code == 400
    assert cl.worker_quotient_finish(10 ** 9, 3).status_code == 400
    r = cl.worker_quotient_finish(acc, 3)
    assert r.status_code == 200 and len(r.json()["commitments"]) == 3 and eng.calls[-1] == ("finish", acc, 3)
    assert cl.worker_quotient_finish(acc, 3).status_code == 400          # consumed
    # an unfinished accumulator is released like a set
    acc2 = cl.worker_quotient_part([a], TERMS).json()["acc"]
    assert cl.worker_release_rows(acc2).status_code == 200 and cl.worker_quotient_finish(acc2, 3).status_code == 400
    assert Client(engine=None).worker_quotient_part([a], TERMS).status_code == 503


def test_client_chain_over_a_fake_engine():
    eng = FakeEngine()
    cl = Client(engine=eng)
    cl.machines_scale, cl._slice_of = 2, None   # what start() leaves for a synthetic setup
    w = cl.worker_commit_rows(0, polys(2, 8, 2)).json()["handle"]
    s = cl.worker_commit_rows(0, polys(2, 8, 3)).json()["handle"]
    r = cl.worker_commit_grand_product_chain([w], [s], [fr(1), fr(7)], fr(3), fr(5), 5, [fr(8), fr(9)], fr(11))
    assert r.status_code == 200 and r.json()["closing"] == fr(11)
    assert eng.calls[-1][5:] == (5, ((8).to_bytes(32, "big"), (9).to_bytes(32, "big")), (11).to_bytes(32, "big"))
    bad = be32_to_fr(R.to_bytes(32, "big"))
    assert cl.worker_commit_grand_product_chain([w], [s], [fr(1), fr(7)], fr(3), fr(5), 5, [], fr(0)).status_code == 400
    assert cl.worker_commit_grand_product_chain([w], [s], [fr(1), fr(7)], fr(3), fr(5), 5, [], bad).status_code == 400
    assert cl.worker_commit_grand_product_chain([w], [s], [], fr(3), fr(5), 5, [], fr(1)).status_code == 400
    assert cl.worker_commit_grand_product_chain([w], [s], [fr(1), fr(7)], fr(3), fr(5), -1, [], fr(1)).status_code == 400


def test_multi_device_client_routes_parts_by_owner():
    engines = [FakeEngine() for _ in range(2)]
    multi = MultiDeviceClient(devices=[0, 1], seed=5, engines=engines)
    multi.start(scale=7, machines_scale=2)
    try:
        a = multi.worker_commit_rows(1, polys(3, 8, 4)).json()["handle"]
        b = multi.worker_commit_rows(2, polys(3, 8, 5)).json()["handle"]
        r = multi.worker_quotient_part([a], TERMS)
        assert r.status_code == 200
        acc = r.json()["acc"]
        owner = multi._row_owner[a]
        assert multi._row_owner[acc] == owner
        assert multi.worker_quotient_part([a], TERMS, acc=acc).status_code == 200
        if multi._row_owner[b] != owner:
            assert multi.worker_quotient_part([b], TERMS, acc=acc).status_code == 400     # another worker's sets
        assert multi.worker_quotient_part([10 ** 9], TERMS).status_code == 400
        r = multi.worker_quotient_finish(acc, 2)
        assert r.status_code == 200 and multi._row_owner[r.json()["handle"]] == owner and acc not in multi._row_owner
        assert multi.worker_quotient_finish(acc, 2).status_code == 400
        s = multi.worker_commit_rows(1, polys(3, 8, 6)).json()["handle"]
        r = multi.worker_commit_grand_product_chain([a], [s], [fr(1), fr(7), fr(49)], fr(3), fr(5), 5, [fr(8), fr(9)], fr(2))
        assert r.status_code == 200 and multi._row_owner[r.json()["handle"]] == owner
    finally:
        multi.stop()
