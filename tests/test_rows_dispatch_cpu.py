"""Every public row-set builder of HipEngine reaches the native export of its OWN name, with that export's argument count,
and refuses a bad shape under its own name before any native call.  No device: the engine is built without __init__ over a
stub library that records calls and answers KZG_OK.  This is the guard that folding the variants onto one private body per
builder did not send them all through one export (the _sel one, say)."""
import ctypes

import pytest

from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet

T, USABLE = 8, 6
S = bytes(31) + b"\x01"                      # a 32-byte scalar
TAIL = [S] * (T - USABLE - 1)


class _Recorder:
    """a library whose every attribute is a function that records its call and returns KZG_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return _native.KZG_OK
        return fn


@pytest.fixture
def eng():
    e = HipEngine.__new__(HipEngine)
    e._lib, e._h, e._set_len, e.verifier = _Recorder(), ctypes.c_void_p(1), {}, None
    return e


def _sets(e, n, first=1):
    return [RowSet(e, first + j, 3, 1, T, [bytes(48)]) for j in range(n)]


PERM = {"wires": [0], "sigmas": [1], "z": 2, "shifts": [S], "beta": S, "gamma": S, "alpha": S}
LOOKUP = {"inputs": [0], "table": [1], "mult": 2, "sum": 3, "width": 1, "theta": S, "beta": S, "alpha": S}
TERMS = [(S, [0, 1])]

# method -> (arguments of a good call, arguments of a call with a bad shape); `h` makes handles: bare integers for the plain
# forms (the engine does not know their row length), RowSet objects for the forms that need it
CASES = {
    "commit_grand_product": lambda h: ((h(2), h(2), [S, S], S, S), (h(2), h(2), [], S, S)),
    "commit_grand_product_zk": lambda h: ((h(2), h(2), [S, S], S, S, USABLE, TAIL), (h(2), h(2), [], S, S, USABLE, TAIL)),
    "commit_grand_product_chain": lambda h: ((h(2), h(2), [S, S], S, S, USABLE, TAIL, S),
                                            (h(2), h(2), [], S, S, USABLE, TAIL, S)),
    "commit_lookup_sum": lambda h: ((h(2), h(1), h(1)[0], 2, 1, S, S), (h(2), h(1), h(1)[0], 0, 1, S, S)),
    "commit_lookup_sum_zk": lambda h: ((h(2), h(1), h(1)[0], 2, 1, S, S, USABLE, TAIL),
                                      (h(2), h(1), h(1)[0], 0, 1, S, S, USABLE, TAIL)),
    "commit_lookup_sum_sel": lambda h: ((h(2), h(1), h(1)[0], h(1), [0, None], 2, 1, S, S, USABLE, TAIL),
                                       (h(2), h(1), h(1)[0], h(1), [], 0, 1, S, S, USABLE, TAIL)),
    "commit_multiplicities": lambda h: ((h(2), h(1), 2, 1), (h(2), h(1), 0, 1)),
    "commit_multiplicities_zk": lambda h: ((h(2), h(1), 2, 1, USABLE, TAIL), (h(2), h(1), 0, 1, USABLE, TAIL)),
    "commit_multiplicities_sel": lambda h: ((h(2), h(1), h(1), [0, None], 2, 1, USABLE, TAIL),
                                           (h(2), h(1), h(1), [], 0, 1, USABLE, TAIL)),
    # the quotient family and SHPLONK: not folded here, held to the same rule.  A bad shape there is an empty constraint
    # system, or no coefficient
    "commit_quotient": lambda h: ((h(3), TERMS, PERM), (h(3), [], None)),
    "commit_quotient_ext": lambda h: ((h(4), TERMS, PERM, LOOKUP), (h(4), [], None, None)),
    "commit_quotient_zk": lambda h: ((h(5), TERMS, PERM, LOOKUP, 4), (h(5), [], None, None, 4)),
    "commit_quotient_sel": lambda h: ((h(5), TERMS, PERM, LOOKUP, [4]), (h(5), [], None, None, [4])),
    "quotient_part": lambda h: ((h(4), TERMS, PERM, LOOKUP), (h(4), [], None, None)),
    "quotient_part_sel": lambda h: ((h(5), TERMS, PERM, LOOKUP, [4]), (h(5), [], None, None, [4])),
    "commit_shplonk": lambda h: ((h(2), [S], [[0, 1]], [S, S]), (h(2), [S], [[0, 1]], [])),
}
PLAIN = {"commit_grand_product", "commit_lookup_sum", "commit_multiplicities"}


@pytest.mark.parametrize("method", sorted(CASES))
def test_a_builder_calls_the_export_of_its_own_name(eng, method):
    bare = method in PLAIN
    handles = (lambda n: list(range(100, 100 + n))) if bare else (lambda n: _sets(eng, n))
    good, bad = CASES[method](handles)

    with pytest.raises(_native.KzgError) as err:
        getattr(eng, method)(*bad)
    assert str(err.value).split(": ", 1)[1].startswith(method + ": "), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"

    out = getattr(eng, method)(*good)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_" + method]
    assert len(eng._lib.calls[0][1]) == len(_native.SYMBOLS["kzg_rows_" + method][1])
    if method == "commit_grand_product_chain":   # ... beta, gamma, usable, tail, start, then the three outputs
        args = eng._lib.calls[0][1]
        assert args[-4] == good[-1] and args[-6] == USABLE and args[-5] == b"".join(TAIL)
    if bare:   # handles of unknown row length are accepted by the plain forms: the set returned knows neither worker nor T
        assert (out[0].i, out[0].T) == (None, None)


def test_the_table_covers_every_variant_of_the_folded_builders():
    for stem in ("commit_grand_product", "commit_lookup_sum", "commit_multiplicities"):
        public = {m for m in dir(HipEngine) if m.startswith(stem)}
        assert public <= set(CASES) and len(public) == 3, public
