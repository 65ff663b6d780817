"""The NTT's pass plans without a device: the library's plan function (kzg_test_ntt_plan_of) is the launcher arithmetic it had
before plan and execution were separated, every plan it makes satisfies the kernels' preconditions, the small plans of
tests/ntt_ref.py cover every per-workgroup geometry those plans hold, the closed forms and the C oracle agree with the transform
summed by its definition, and kzg_test_ntt_run refuses a malformed plan before it looks at its context."""
import ctypes

import pytest

from oracle import cpu as oc
from oracle.bls12_381 import R
from tests import ntt_ref as nr
from zkp_subnet_amd import _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.engine import ntt_plan_of


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def launcher_arithmetic(log_n, radix2, tile_log):
    """The two loops of launch_fr_ntt / launch_fr_ntt_radix2 as they stood before the split, transcribed line by line:
    ceil(log_n / max_s) passes of near-equal depth; columns = what the tile allows, bounded by what exists (tiles in the
    first pass, s0 low bits later); the first pass takes at most 4 tiles."""
    tile, max_s = (10, 8) if radix2 else (tile_log, tile_log - 2)
    passes = (log_n + max_s - 1) // max_s
    out, s0 = [], 0
    for p in range(passes):
        S = (log_n - s0 + (passes - p) - 1) // (passes - p)
        logC = tile - S
        avail = log_n - S if p == 0 else s0
        if logC > avail:
            logC = avail
        if p == 0 and logC > 2:
            logC = 2
        out.append((S, logC))
        s0 += S
    return out


def test_plan_function_is_the_launcher_arithmetic_it_replaced(lib, monkeypatch):
    monkeypatch.delenv("KZG_NTT_RADIX2", raising=False)
    monkeypatch.delenv("KZG_NTT_TILE_LOG", raising=False)
    for log_n in range(1, 29):
        for tile_log in (8, 9, 10, 11):
            assert ntt_plan_of(log_n, 0, tile_log) == (0, launcher_arithmetic(log_n, False, tile_log)), (log_n, tile_log)
            assert ntt_plan_of(log_n, 1, tile_log) == (1, launcher_arithmetic(log_n, True, tile_log)), (log_n, tile_log)
        # what production picks: the radix-2 kernel below 2^18, the register-blocked one with 1024-element tiles from there
        want = (1, launcher_arithmetic(log_n, True, 10)) if log_n < 18 else (0, launcher_arithmetic(log_n, False, 10))
        assert ntt_plan_of(log_n) == want == ntt_plan_of(log_n, -1, 0), log_n
        assert ntt_plan_of(log_n, 0, 0) == (0, launcher_arithmetic(log_n, False, 10))
    # the shapes DESIGN 3.4 quotes
    assert ntt_plan_of(22) == (0, [(8, 2), (7, 3), (7, 3)]) and ntt_plan_of(22, 1) == (1, [(8, 2), (7, 3), (7, 3)])
    assert ntt_plan_of(22, 0, 11) == (0, [(8, 2), (7, 4), (7, 4)]) and ntt_plan_of(18, 0, 11)[1][0][0] == 9
    assert ntt_plan_of(9, 1) == (1, [(5, 2), (4, 5)]) and ntt_plan_of(8, 1) == (1, [(8, 0)])


_KNOBS = r'''
import sys
sys.path.insert(0, %r)
from zkp_subnet_amd.engine import ntt_plan_of
print([ntt_plan_of(lg) for lg in (9, 17, 18, 22)])
'''


def test_the_two_environment_knobs_still_steer_the_production_plan(lib):
    """KZG_NTT_RADIX2 / KZG_NTT_TILE_LOG are read once per process: each setting in an interpreter of its own (no device)."""
    import os
    import subprocess
    import sys

    from tests.gpu_common import ROOT

    def run(**env):
        base = {k: v for k, v in os.environ.items() if k not in ("KZG_NTT_RADIX2", "KZG_NTT_TILE_LOG")}
        out = subprocess.run([sys.executable, "-c", _KNOBS % ROOT], capture_output=True, text=True, timeout=300, env=dict(base, **env))
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.strip()

    def want(radix2_from, tile_log):
        return str([(1, launcher_arithmetic(lg, True, 10)) if lg < radix2_from else (0, launcher_arithmetic(lg, False, tile_log))
                    for lg in (9, 17, 18, 22)])

    assert run() == want(18, 10)
    assert run(KZG_NTT_RADIX2="1") == want(99, 10)
    assert run(KZG_NTT_TILE_LOG="11") == want(18, 11) and run(KZG_NTT_TILE_LOG="9") == want(18, 9)
    assert run(KZG_NTT_TILE_LOG="12") == want(18, 10) and run(KZG_NTT_RADIX2="0") == want(18, 10)      # out of range: ignored


def test_every_production_plan_satisfies_the_kernels_preconditions(lib):
    for log_n in range(1, 29):
        for kernel in (0, 1):
            for tile_log in (8, 9, 10, 11):
                form, passes = ntt_plan_of(log_n, kernel, tile_log)
                assert nr.plan_invalid(log_n, form, passes) is None, nr.plan_name(log_n, form, passes)
                assert all(S + logC <= (10 if kernel else tile_log) for S, logC in passes)
    for bad in ((0, -1, 0), (32, -1, 0), (10, 2, 0), (10, -2, 0), (10, 0, 7), (10, 0, 12)):
        arr = (ctypes.c_int * 8)()
        assert lib.kzg_test_ntt_plan_of(*bad, arr, arr, ctypes.byref(ctypes.c_int())) == _native.KZG_E_ARG, bad
    assert lib.kzg_test_ntt_plan_of(10, -1, 0, None, None, None) == _native.KZG_E_ARG


def test_covering_plans_hold_every_production_geometry_at_small_sizes(lib):
    tuples = nr.production_tuples()
    cover = nr.covering_plans()
    held = set()
    for log_n, kernel, passes in cover:
        assert nr.plan_invalid(log_n, kernel, passes) is None and log_n <= 13, nr.plan_name(log_n, kernel, passes)
        held.update(nr.plan_tuples(kernel, passes))
    assert tuples <= held, sorted(tuples - held)
    # what the sizes 2^17 .. 2^22 reached one at a time: nine- and eight-stage passes in every position, odd and even S,
    # the 64- / 128-lane instantiations (tiles of at most 256 / 512 elements) and the 512-lane one
    for t in ((0, "first", 9, 2), (0, "last", 9, 2), (0, "middle", 9, 2), (0, "first", 8, 2), (0, "middle", 8, 2), (0, "only", 9, 0),
              (1, "first", 8, 2), (1, "middle", 7, 3), (1, "last", 7, 3), (1, "only", 8, 0)):
        assert t in tuples, t
    quads = {(1 << (S + logC)) >> 2 for k, _, S, logC in tuples if k == 0}
    assert {q > 256 for q in quads} == {True, False} and any(q <= 64 for q in quads) and any(64 < q <= 128 for q in quads)
    # the smallest size is the smallest: no plan of a smaller log_n holds the geometry
    for log_n, kernel, passes in cover:
        for t in set(nr.plan_tuples(kernel, passes)) & tuples:
            assert nr.smallest_plan_with(t)[0] <= log_n
    for kernel in (0, 1):
        for t in (x for x in tuples if x[0] == kernel):
            lg = nr.smallest_plan_with(t)[0]
            for smaller in range(1, min(lg, 7)):          # (exhaustively where the list of all plans is short)
                assert all(t not in nr.plan_tuples(kernel, pl) for pl in nr.valid_plans(smaller, kernel)), (t, smaller)


def test_valid_plans_are_exactly_the_plans_the_library_accepts(lib):
    """the Python restatement of the preconditions and the library's agree on every candidate plan of 2^1 .. 2^4 with S in 0 .. 5
    and logC in -1 .. 5 -- read from the refusal: a valid plan with no context is refused for the context, not for the plan"""
    import itertools

    for kernel in (0, 1):
        for log_n in (1, 2, 3, 4):
            listed = set(nr.valid_plans(log_n, kernel))
            for passes in (1, 2, 3):
                for S in itertools.product(range(0, 6), repeat=passes):
                    if sum(S) != log_n and passes == 3:
                        continue
                    for logC in itertools.product(range(-1, 6), repeat=passes):
                        plan = tuple(zip(S, logC))
                        ok = _refusal(lib, log_n, kernel, plan) == b"ntt plan: no context or no data"
                        assert ok == (nr.plan_invalid(log_n, kernel, plan) is None) == (plan in listed), (log_n, kernel, plan)


def test_closed_forms_and_the_c_oracle_equal_the_transform_by_definition():
    oc.build()
    assert nr.root(1) == R - 1 and pow(nr.root(8), 256, R) == 1 and pow(nr.root(8), 128, R) == R - 1
    for log_n in range(0, nr.DEF_MAX_LOG + 1):
        fams = nr.families(log_n)
        assert {"zero", "constant r-1", "alternating", "edge pool", "uniform", f"delta r-1 at {(1 << log_n) - 1}"} <= set(fams)
        for f in fams.values():
            assert len(f.a) == 1 << log_n and all(0 <= v < R for v in f.a)
            for inverse in (False, True):
                by_def = nr.ntt_by_definition(f.a, inverse)
                c = f.closed(inverse)
                assert c is None or c == by_def, (log_n, f.name, inverse)
                assert list(f.expected(inverse)) == by_def
                raw = oc.fr_ntt(nr.to_bytes(f.a), inverse)
                assert raw == nr.to_bytes(by_def), (log_n, f.name, inverse)
            assert nr.ntt_by_definition(nr.ntt_by_definition(f.a), True) == f.a
    # above 2^8 the reference is the oracle's: its closed forms keep holding there
    for name, f in nr.families(11).items():
        for inverse in (False, True):
            c = f.closed(inverse)
            assert c is None or nr.to_bytes(c) == oc.fr_ntt(nr.to_bytes(f.a), inverse), (name, inverse)


def test_lazy_model_of_a_pass_holds_what_the_documents_quote(capsys):
    """scripts/models/ntt_lazy_model.py (its own assertions): the zero vector ends at r (3S + 1) through the representatives 0 and
    r of zero, and limbs and accumulators are bounded for every input at normalisation periods 2 and 3, not at 4"""
    import importlib.util
    import os
    import sys

    from tests.gpu_common import ROOT

    spec = importlib.util.spec_from_file_location("ntt_lazy_model", os.path.join(ROOT, "scripts", "models", "ntt_lazy_model.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
        mod.main()
    finally:
        sys.path[:] = path
    assert "ntt lazy model ok" in capsys.readouterr().out
    assert mod.worst_case(3)[0] < 1 << 32 and mod.worst_case(3)[1] < 1 << 64 <= mod.worst_case(4)[1]


def _refusal(lib, log_n, kernel, plan, ctx=None, data=True):
    buf = ctypes.create_string_buffer(32 << max(log_n, 0)) if data else None
    n = len(plan)
    S, logC = (ctypes.c_int * max(n, 1))(*[p[0] for p in plan]), (ctypes.c_int * max(n, 1))(*[p[1] for p in plan])
    rc = lib.kzg_test_ntt_run(ctx, ctypes.addressof(buf) if data else None, log_n, 0, kernel, n, S, logC)
    assert rc == _native.KZG_E_ARG, (log_n, kernel, plan, rc)
    return lib.kzg_last_error(None)


def test_run_hook_refuses_a_null_context_and_every_malformed_plan_without_a_device(lib):
    lib.kzg_last_error.restype = ctypes.c_char_p
    none = b"ntt plan: no context or no data"
    # a valid plan gets as far as the context, and no further
    for kernel in (0, 1):
        for log_n in (1, 5, 10, 13):
            form, passes = ntt_plan_of(log_n, kernel, 10)
            assert _refusal(lib, log_n, form, passes) == none
    assert _refusal(lib, 11, 0, [(9, 2), (2, 9)]) == none and _refusal(lib, 11, 1, [(2, 2), (8, 2), (1, 9)]) == none
    sums, fit, cols, stages = (b"ntt plan: the stages do not sum to log_n", b"ntt plan: a pass does not fit the tile",
                               b"ntt plan: more columns than the pass has",
                               b"ntt plan: a pass has fewer than 1 or more stages than its kernel admits")
    for kernel in (0, 1):
        assert _refusal(lib, 10, kernel, [(5, 2), (4, 2)]) == sums                 # a sum other than log_n: short
        assert _refusal(lib, 10, kernel, [(5, 2), (6, 2)]) == sums                 # ... and long
        assert _refusal(lib, 10, kernel, [(5, 2), (5, 2), (1, 0)]) == sums
        assert _refusal(lib, 10, kernel, [(0, 2), (5, 2), (5, 2)]) == stages       # S = 0
        assert _refusal(lib, 10, kernel, [(5, 2), (0, 2), (5, 2)]) == stages
        assert _refusal(lib, 10, kernel, [(10, 0)]) == stages                      # S = 10
        assert _refusal(lib, 12, kernel, [(2, 2), (10, 0)]) == stages
        assert _refusal(lib, 10, kernel, [(-3, 0), (13, 0)]) == stages
        assert _refusal(lib, 10, kernel, [(5, 2), (5, -1)]) == fit                 # a negative column count
        assert _refusal(lib, 10, kernel, [(2, 2), (4, 3), (4, 2)]) == cols         # logC > s0
        assert _refusal(lib, 6, kernel, [(1, 1), (5, 2)]) == cols
        assert _refusal(lib, 10, kernel, [(4, 2), (3, 5), (3, 2)]) == cols
        assert _refusal(lib, 10, kernel, [(7, 4), (3, 2)]) == (fit if kernel else cols)    # first pass: logC > log_n - S
        assert _refusal(lib, 3, kernel, [(2, 2), (1, 0)]) == cols
        assert _refusal(lib, 10, kernel, []) == b"ntt plan: number of passes outside [1, 8]"       # passes = 0
        assert _refusal(lib, 9, kernel, [(1, 0)] * 9) == b"ntt plan: number of passes outside [1, 8]"
        assert _refusal(lib, 0, kernel, [(1, 0)]) == b"ntt plan: log_n outside [1, 22]"
        assert _refusal(lib, 23, kernel, [(8, 2), (8, 2), (7, 2)]) == b"ntt plan: log_n outside [1, 22]"
    # logC beyond the tile: 2^10 elements for the radix-2 kernel, 2^11 for the register-blocked one; S = 9 only for the latter
    assert _refusal(lib, 16, 1, [(8, 2), (8, 3)]) == fit and _refusal(lib, 16, 1, [(8, 2), (8, 2)]) == none
    assert _refusal(lib, 16, 0, [(8, 2), (8, 4)]) == fit and _refusal(lib, 16, 0, [(8, 2), (8, 3)]) == none
    assert _refusal(lib, 18, 0, [(9, 3), (9, 2)]) == fit and _refusal(lib, 18, 0, [(9, 2), (9, 2)]) == none
    assert _refusal(lib, 18, 1, [(9, 1), (9, 1)]) == stages
    assert _refusal(lib, 20, 0, [(5, 2), (5, 5), (5, 7), (5, 6)]) == fit
    for kernel in (-1, 2):
        assert _refusal(lib, 10, kernel, [(5, 2), (5, 2)]) == b"ntt plan: kernel must be 0 (register-blocked) or 1 (radix-2)"
    assert _refusal(lib, 10, 1, [(5, 2), (5, 2)], data=False) == none
    S = (ctypes.c_int * 2)(5, 5)
    buf = ctypes.create_string_buffer(32 << 10)
    assert lib.kzg_test_ntt_run(None, ctypes.addressof(buf), 10, 0, 1, 2, None, S) == _native.KZG_E_ARG
    assert lib.kzg_test_ntt_run(None, ctypes.addressof(buf), 10, 0, 1, 2, S, None) == _native.KZG_E_ARG
    assert buf.raw == bytes(32 << 10)
