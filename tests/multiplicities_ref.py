"""The multiplicity row of kzg_rows_commit_multiplicities from its definition, in Python -- the reference of
tests/test_multiplicities_cpu.py (which pins it against a brute force) and tests/test_gpu_multiplicities.py (which compares
the GPU with it)."""


def multiplicities(inputs, table, n_lookups, width):
    """(mult, missing): inputs holds n_lookups * width lists of T field elements (lookup-major), table width lists.
    mult[t] = how many input cells (l, t') carry a tuple whose FIRST occurrence in the table is row t; missing = how many
    carry a tuple that is no row of the table.  Tuples are compared in all width columns."""
    assert len(inputs) == n_lookups * width and len(table) == width
    T = len(table[0])
    first = {}
    for t in range(T):
        first.setdefault(tuple(col[t] for col in table), t)
    mult, missing = [0] * T, 0
    for l in range(n_lookups):
        cols = inputs[l * width:(l + 1) * width]
        for t in range(T):
            at = first.get(tuple(col[t] for col in cols))
            if at is None:
                missing += 1
            else:
                mult[at] += 1
    return mult, missing
