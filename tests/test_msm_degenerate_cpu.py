"""The reference of tests/test_gpu_msm_degenerate.py checked WITHOUT the code under test (no GPU): the known-log expectation
against the C oracle's MSM over the same bytes, the digit / bucket / tree model against the plain sum, and every case's
census precondition at every shape -- a case that cannot meet its precondition is changed here, before it reaches a GPU."""
from collections import Counter

import pytest

from oracle import bls12_381 as o
from oracle import cpu as oc
from tests import degenerate_ref as dr

R = o.R


@pytest.fixture(scope="module")
def records():
    cache = {}

    def of(logs):
        for k in set(logs) - set(cache):
            cache[k] = dr.record(k)
        return b"".join(cache[k] for k in logs)

    return of


@pytest.mark.parametrize("tau", list(dr.TAUS))
def test_special_tau_point_sets_are_what_the_oracle_generates(records, tau):
    oc.build()
    srs = oc.srs_gen(dr.TAUS[tau].to_bytes(32, "big"), (1).to_bytes(32, "big"), 10, 0, 0)
    logs = dr.tau_logs(dr.TAUS[tau], 1 << 10)
    assert srs == records(logs)
    assert len(set(logs)) == {"one": 1, "minus_one": 2, "zero": 2, "fourth_root": 4}[tau]
    if tau == "minus_one":
        assert oc.msm(srs, (12345).to_bytes(32, "big") * (1 << 10)) == o.g1_compress(None)


def test_pool_records_and_arranged_order():
    assert [o.g1_from_be96(r) for r in dr.POOL_RECORDS] == [o.g1_mul(o.G1, k) if k else None for k in dr.POOL_LOGS]
    assert dr.POOL_RECORDS[3] == bytes(96) and dr.POOL_RECORDS[2] == o.g1_to_be96(o.g1_neg(o.G1))
    rec, logs = dr.pool_srs(64, 7, arranged=True)
    assert logs[:16] == [0] * 16 and logs[16:32] == [5] * 16 and rec[:96 * 16] == bytes(96 * 16)
    assert len(set(dr.pool_srs(4096, 4096)[1])) == 6


@pytest.mark.parametrize("lg", [10, 12])
@pytest.mark.parametrize("kind", dr.SRS_KINDS)
def test_expected_equals_the_oracle_msm_over_the_same_bytes(records, lg, kind):
    """expected() (one fixed-base multiplication) == oc.msm (a Pippenger MSM of its own) for every point source and scalar
    family of the GPU module; the buckets' weighted sum and the tree's root identity give the same log."""
    oc.build()
    n = 1 << lg
    logs, rec = dr.srs_logs(kind, n, want_records=True)
    srs = rec if rec is not None else records(logs)
    offsets = dr.window_offsets(lg)
    for fam in dr.FAMILIES:
        sc = dr.family(fam, n, offsets, seed=lg)
        assert all(0 <= s < R for s in sc)
        want = dr.expected(sc, logs)
        assert want == oc.msm(srs, o.fr_to_be32(sc), threads=8), (kind, fam)
        total = sum(s * k for s, k in zip(sc, logs)) % R
        blogs = dr.bucket_logs(sc, logs, offsets)
        assert sum((i + 1) * b for i, b in enumerate(blogs)) % R == total, (kind, fam)
        levels, roots = dr.tree_census(blogs)
        assert len(roots) == 1 and len(roots[0]) == len(levels) + 1 and dr.root_value(roots[0]) == total, (kind, fam)
    # ragged length and offset, logs sliced alike
    m, off = n - 3, 2
    assert dr.expected(sc[:m], logs[off:off + m]) == oc.msm(srs[96 * off:96 * (off + m)], o.fr_to_be32(sc[:m]), threads=8)


def test_digits_restate_the_signed_recode():
    for lg, window in dr.SHAPES + ((10, 24),):
        offsets = dr.window_offsets(lg, window)
        assert offsets[0] == 0 and offsets[-1] == 256 and max(b - a for a, b in zip(offsets, offsets[1:])) == \
            (window or dr.choose_window(lg))
        sc = dr.family("uniform", 64, offsets, seed=lg) + dr.EDGE_POOL + list(dr.paired_scalars(offsets))
        arr = dr.digit_array(sc, offsets)
        for j, s in enumerate(sc):
            d = dr.digits(s, offsets)
            assert d == list(arr[j])
            assert sum(x << off for x, off in zip(d, offsets)) == s
            assert all(-(1 << (b - a - 1)) < x <= 1 << (b - a - 1) for x, a, b in zip(d, offsets, offsets[1:]))
    # a digit above half goes negative and carries; exactly half stays positive
    assert dr.digits((1 << 9) + (3 << 10), [0, 10, 20, 256])[:2] == [512, 3]
    assert dr.digits((1 << 9) + 1 + (3 << 10), [0, 10, 20, 256])[:2] == [-511, 4]


def test_tree_census_classes_and_two_roots():
    levels, roots = dr.tree_census([5, 5, 7, R - 7, 0, 3, 0, 0])
    assert [(x["ops"], x["dbl"], x["cancel"], x["inf"]) for x in levels] == [(4, 1, 1, 2), (4, 0, 0, 3), (3, 0, 0, 1)]
    assert dr.root_value(roots[0]) == (5 + 2 * 5 + 3 * 7 - 4 * 7 + 6 * 3) % R
    levels, roots = dr.tree_census([1, 2, 3, 4, 10, 20, 30, 40], stop=2)          # two bucket sets, two roots
    assert len(levels) == 2 and [dr.root_value(r) for r in roots] == [1 + 4 + 9 + 16, 10 + 40 + 90 + 160]
    assert [dr.classify(x) for x in (1, 3072, 3073, 32768, 32769)] == ["lp", "lp", "coop", "coop", "wide"]
    assert [dr.pick_chunk(x) for x in (1, 26624, 90112, 1 << 21, (1 << 17) * 20)] == [6, 6, 6, 32, 20]


@pytest.mark.parametrize("kind", dr.SRS_KINDS)
@pytest.mark.parametrize("lg,window", dr.SHAPES)
def test_every_case_meets_its_census_precondition(lg, window, kind):
    cases = [f for k, f in dr.cases_of(lg, window) if k == kind]
    assert cases or (lg == 17 and kind.startswith("pool"))
    for fam in cases:
        case = dr.build_case(lg, window, kind, fam)
        failed = [what for what, ok in dr.preconditions(case) if not ok]
        assert not failed, (lg, window, kind, fam, failed, case.fold["kernels"])


@pytest.mark.parametrize("kind,fam", [("one", "equal"), ("zero", "equal"), ("zero", "uniform"), ("pool", "uniform"),
                                      ("pool_arranged", "equal"), ("minus_one", "paired")])
def test_case_facts_against_an_entry_by_entry_accumulate(kind, fam):
    """What a Case derives with array passes (entries per bucket, sum s_j k_j, the fold's plan and its certain facts), redone
    the slow way: every entry listed, sorted by bucket in (window, point) order, cut into chunks, carries summed as integers."""
    lg, window = 10, 0
    c = dr.build_case(lg, window, kind, fam)
    assert c.scalar_bytes == o.fr_to_be32(c.scalars) and c.total == sum(s * k for s, k in zip(c.scalars, c.logs)) % R
    assert c.expected == dr.expected(c.scalars, c.logs)
    entries = [(abs(d) - 1, ((k if d > 0 else R - k) << c.offsets[w]) % R if k else None)
               for w in range(c.nwin) for s, k in zip(c.scalars, c.logs) for d in [dr.digits(s, c.offsets)[w]] if d]
    entries.sort(key=lambda e: e[0])
    per_bucket, infinite = Counter(b for b, _ in entries), Counter(b for b, v in entries if v is None)
    assert [per_bucket[i] for i in range(c.nbuckets)] == list(c.counts)
    assert [infinite[i] for i in range(c.nbuckets)] == list(c.inf_counts)
    sums = [0] * c.nbuckets
    for b, v in entries:
        sums[b] = (sums[b] + (v or 0)) % R
    assert sums == c.buckets.logs
    chunk = c.fold["chunk"]
    assert chunk == dr.pick_chunk(c.n * c.nwin) == 6 and c.fold["nchunks"] == -(-c.n * c.nwin // chunk)
    carries = {}                              # bucket -> [(sum, finite entries, entries)] of the chunks its run continues into
    for t in range(0, len(entries), chunk):
        b = entries[t][0]
        if t and entries[t - 1][0] == b:     # the chunk's first run began in an earlier chunk: a carry
            part = [v for bb, v in entries[t:t + chunk] if bb == b]
            carries.setdefault(b, []).append((sum(v or 0 for v in part) % R, sum(v is not None for v in part), len(part)))
    assert [len(carries.get(i, [])) for i in range(c.nbuckets)] == list(c.fold["runs"])
    longest = max(len(v) for v in carries.values())
    assert c.fold["max_run"] == (longest if longest > 1 else 0)
    assert (c.fold["kernels"] == ["k_fold_bucket_lp"]) == (longest <= dr.KZG_FOLD_BUCKET_RUN)
    # the certain facts are lower bounds of what this order shows
    assert sum(1 for v in carries.values() for _, finite, _ in v if finite == 0) >= c.fold["fold_inf_carries"]
    assert c.fold["acc_inf_runs"] == sum(1 for i in range(c.nbuckets) if c.counts[i] and c.counts[i] == c.inf_counts[i])
    doubling_pairs = sum(1 for v in carries.values() for i in range(0, len(v) - 1, 2)
                         if v[i][0] == v[i + 1][0] != 0 and v[i][2] == v[i + 1][2] == chunk)
    assert doubling_pairs >= c.runs["same_pairs"]
    if (kind, fam) == ("one", "equal"):
        assert c.runs["same_pairs"] >= c.nwin
