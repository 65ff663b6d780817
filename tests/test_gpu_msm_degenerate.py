"""GPU parity tests (`-m gpu`), msm over repeated, opposite and infinite points: the exceptional branches of every point
addition (equal operands -> doubling, opposite -> infinity, an infinite operand) executed INSIDE a pipeline with carries, a
fold and a real bucket tree.  All points are multiples [k_j]G with k_j known (tests/degenerate_ref.py), so every expected
value is one fixed-base multiplication of the oracle and every check is bit-exact.  Each case first asserts, on the integer
model of the pipeline, that it reaches the kernels and contains the exceptional additions it is there for
(degenerate_ref.preconditions; checked without a GPU by tests/test_msm_degenerate_cpu.py).

Shapes (n = 2^lg points, nwin windows, B = 2^(c-1) buckets, entries = n * nwin, chunk = pick_chunk(entries),
nchunks = ceil(entries / chunk); tree level L has (B >> (L + 1)) * (L + 1) additions: > 32768 wide (k_msm_tree_level),
<= 3072 lane-parallel (k_msm_tree_level_lp, two levels per launch as k_msm_tree_level2_lp), else cooperative):

  lg  window  c  nwin  B       entries  chunk nchunks  fold                                   tree additions per level
  10  0       10 26    512     26624    6     4438     uniform: ~9 carries per run (<= 24)    256 256 192 128 80 48 28 16 | 9
                                                       and B <= 4096 -> k_fold_bucket_lp      four paired launches + one single
  12  0       12 22    2048    90112    6     15019    equal: runs of 683 carries, 10 steps:  1024 1024 768 ... : all lane-parallel
                                                       nchunks/2d > 3072 for d = 1, 2 ->
                                                       k_fold_step_coop, then k_fold_step_lp;
                                                       nchunks <= 65536 -> k_fold_heads_coop
  12  16      16 16    32768   65536    6     10923    as above                               16384 16384 12288 8192 5120 cooperative,
                                                                                              then 3072 ... lane-parallel
  11  18      18 15    131072  30720    6     5120     as above                               65536 65536 49152 wide (64 | n_out: the
                                                                                              LDS-staged store), 32768 ... 4096
                                                                                              cooperative, then lane-parallel
  17  13      13 20    4096    2621440  20    131072   entries > 2^21 -> 131072 chunks        2048 2048 1536 ... : all lane-parallel
                                                       > 65536 -> k_fold_step / k_fold_heads
                                                       (equal: runs of 6553 carries)

Point sources: the synthetic SRS [tau^j]G with tau = 1 (all G), r - 1 (G, -G, ...), 0 (G, then infinities) and a primitive
fourth root of unity (four points, repeating); a loaded SRS drawn from the pool {G, G, -G, infinity, 5G, -5G, 2G} in seeded
random order, and the same with a block of infinities followed by a block of one point.  Scalar families: uniform, equal (one
scalar whose digits differ from window to window: every bucket run is n copies of one table row), paired (two alternating
scalars with digits 2m + 1 / 2m + 2: adjacent buckets come out equal or opposite, tree level 0 doubles or cancels), edge."""
import pytest

from oracle import bls12_381 as o
from oracle import cpu as oc
from tests import degenerate_ref as dr

pytestmark = pytest.mark.gpu

R = o.R
_RECORD = {}


def records(logs):
    for k in set(logs) - set(_RECORD):
        _RECORD[k] = dr.record(k)
    return b"".join(_RECORD[k] for k in logs)


class Engines:
    """One context per window setting, reloaded when a test needs another SRS (a reload swaps the whole table)."""

    def __init__(self, make):
        self.make, self.made, self.held = make, {}, {}

    def resident(self, window, lg, kind):
        """(engine, logs) with SRS `kind` of 2^lg points resident; what the device holds must be the records of those logs
        (the generator's and the loader's batched affine conversion on infinite points)."""
        if window not in self.made:
            self.made[window] = self.make(window)
        eng, n = self.made[window], 1 << lg
        logs, rec = dr.srs_logs(kind, n, want_records=True)
        if self.held.get(window) != (lg, kind):
            self.held[window] = None
            if rec is None:
                eng.gen_srs(dr.TAUS[kind], 1, lg, 0)
                rec = records(logs)
            else:
                eng.load_srs(rec, lg, 0)
            assert eng.srs_read(0, n) == rec, (lg, kind)
            self.held[window] = (lg, kind)
        return eng, logs


@pytest.fixture(scope="module")
def engine(hip):
    return Engines(hip)


def require(case):
    failed = [what for what, ok in dr.preconditions(case) if not ok]
    assert not failed, (case.lg, case.window, case.kind, case.family, failed, case.fold["kernels"])


@pytest.mark.parametrize("lg,window,kind,fam", [(lg, w, k, f) for lg, w in dr.SHAPES for k, f in dr.cases_of(lg, w)])
def test_msm_over_degenerate_points(engine, lg, window, kind, fam):
    eng, logs = engine.resident(window, lg, kind)
    case = dr.build_case(lg, window, kind, fam)
    require(case)
    assert eng.window_offsets == case.offsets and case.logs == logs
    assert eng.msm(case.scalar_bytes, 0) == case.expected, (lg, window, kind, fam, case.fold["kernels"])


def test_infinity_through_the_whole_pipeline(engine):
    """tau = r - 1, even n, equal scalars: every bucket, carry, tree node and root component is infinity."""
    lg, n = 12, 1 << 12
    eng, logs = engine.resident(0, lg, "minus_one")
    case = dr.build_case(lg, 0, "minus_one", "equal")
    require(case)
    assert not any(case.buckets.logs) and not any(case.roots[0]) and case.total == 0
    sc = case.scalar_bytes
    assert eng.msm(sc, 0) == o.g1_compress(None) == case.expected
    part = eng.msm_partial(sc, 0)
    assert part == bytes(192)
    assert eng.g1_sum(part) == o.g1_compress(None) and eng.g1_sum(part * 3) == o.g1_compress(None)


@pytest.mark.parametrize("kind", ["pool", "pool_arranged"])
def test_ragged_length_and_offset_over_the_pool(engine, kind):
    lg, n = 12, 1 << 12
    eng, logs = engine.resident(0, lg, kind)
    m, off = n - 3, 2
    for fam in ("uniform", "equal"):
        case = dr.build_case(lg, 0, kind, fam, logs=logs[off:off + m], n=m)
        require(case)
        assert eng.msm(case.scalar_bytes, off) == case.expected, (kind, fam)


@pytest.mark.parametrize("lg,window,kind", [(10, 0, "pool"), (10, 16, "pool_arranged"), (10, 0, "zero")])
def test_infinite_rows_in_the_window_tables(engine, lg, window, kind):
    """k_precomp_dbl / k_precomp_norm on infinite points: the row of an infinite point is infinity in every window table,
    its finite neighbour's is 2^off[w] P; an MSM whose slice STARTS at an infinite point is correct."""
    n = 1 << lg
    eng, logs = engine.resident(window, lg, kind)
    offs = eng.window_offsets
    assert offs == dr.window_offsets(lg, window)
    nwin = len(offs) - 1
    j = next(i for i in range(1, n - 1) if logs[i] == 0 and logs[i - 1] != 0)        # infinite, finite neighbour before it
    jj = max(i for i in range(n) if logs[i] == 0)                                    # the last infinite point
    for w in (0, nwin // 2, nwin - 1):
        assert eng.srs_read(j, 1, window=w) == o.g1_to_be96(None) == eng.srs_read(jj, 1, window=w)
        assert eng.srs_read(j - 1, 1, window=w) == dr.record(logs[j - 1] << offs[w]), (w, j)
        assert eng.srs_read(j - 1, 2, window=w)[96:] == bytes(96)
    m = min(n - j, 777)
    case = dr.build_case(lg, window, kind, "uniform", logs=logs[j:j + m], n=m)
    assert case.logs[0] == 0 and case.fold["acc_inf_entries"] >= nwin - 1
    assert eng.msm(case.scalar_bytes, j) == case.expected


@pytest.mark.parametrize("alpha", [0xA1FA << 64, 1, R - 1], ids=["alpha_mid", "alpha_1", "alpha_r_minus_1"])
@pytest.mark.parametrize("kind", ["one", "minus_one"])
def test_two_roots_commit_open_over_repeated_points(engine, kind, alpha):
    """commit + open of one row in one pass: two bucket sets, the tree stops at two nodes.  The row (coefficient form) is
    the equal family, so the commitment's bucket set is the one of the equal case: runs of one repeated row.  For the
    first alpha the pass is also modelled as the tree sees it (the row's buckets, then the quotient's)."""
    lg, n = 12, 1 << 12
    eng, logs = engine.resident(0, lg, kind)
    case = dr.build_case(lg, 0, kind, "equal")
    require(case)
    row, a = case.scalar_bytes, alpha.to_bytes(32, "big")
    srs = oc.srs_gen(dr.TAUS[kind].to_bytes(32, "big"), (1).to_bytes(32, "big"), lg, 0, 0)
    c, ev, pf = eng.commit_open(0, row, a, False)
    assert c == oc.commit(srs, row, False, threads=8) == case.expected, (kind, alpha)
    assert (ev, pf) == oc.open_(srs, row, a, False, threads=8), (kind, alpha)
    if alpha == 0xA1FA << 64:
        y, q = o.poly_quotient(case.scalars, alpha)
        q = (list(q) + [0] * n)[:n]
        levels, roots = dr.tree_census(case.buckets.logs + dr.bucket_logs(q, logs, case.offsets), stop=2)
        assert len(roots) == 2 and len(levels) == len(case.levels)
        assert levels[0]["inf"] >= 1 and all(x["ops"] == 2 * z["ops"] for x, z in zip(levels, case.levels))
        assert ev == y.to_bytes(32, "big") and [c, pf] == [oc.g1_mul_gen(dr.root_value(r).to_bytes(32, "big")) for r in roots]


def test_ticketed_msm_with_a_deep_fold(engine):
    """msm_submit / msm_wait of an equal case (runs of 683 carries, ten fold steps) give the blocking result."""
    lg, n = 12, 1 << 12
    eng, logs = engine.resident(0, lg, "one")
    case = dr.build_case(lg, 0, "one", "equal")
    require(case)
    sc, want = case.scalar_bytes, case.expected
    eng.upload_fr(0, sc, False)
    t1, t2 = eng.msm_submit(0, n, 0), eng.msm_submit(0, n, 0, partial=True)
    assert eng.msm_wait(t1) == want == eng.msm(sc, 0) and eng.g1_sum(eng.msm_wait(t2)) == want
