"""CPU: the normative model of the multicolour ordering (tests/coloring_model.c) is held to account -- against a plain-Python
restatement of the rule over sets, on the properties a colouring must have, on the level counts it promises ILUAM -- and the new
entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from coloring_modellib import Model, key, neighbours, python_coloring, reorder_py
from iluam_modellib import level_schedules
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("coloring_model"))


def csc_of(S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def random_pattern(rng, n, symmetric, density):
    """a random pattern with a full diagonal (what the preconditioner accepts), values 1, 2, 3, ... in stored order"""
    M = rng.random((n, n)) < density
    if symmetric:
        M = M | M.T
    M |= np.eye(n, dtype=bool)
    cp, rv, _ = csc_of(sp.csc_matrix(M.astype(np.float64)))
    return cp, rv, np.arange(1.0, len(rv) + 1)


def patterns():
    rng = np.random.default_rng(40)
    for trial in range(300):
        n = int(rng.integers(1, 17))
        yield trial, n, random_pattern(rng, n, trial % 2 == 0, rng.choice([0.08, 0.2, 0.45]))


def check_coloring(cp, rv, col):
    """proper (no two neighbours share a colour), complete, every colour used, c the vertices by (colour, index)"""
    n = len(cp) - 1
    N = neighbours(cp, rv)
    assert len(col.color) == n and np.all(col.color >= 0) and np.all(col.color < col.ncolors)
    assert all(col.color[i] != col.color[j] for i in range(n) for j in N[i])
    assert np.array_equal(np.sort(col.c), np.arange(n))
    assert np.array_equal(col.c, np.lexsort((np.arange(n), col.color)))
    assert col.ptr[0] == 0 and col.ptr[-1] == n and np.all(np.diff(col.ptr) > 0)
    for r in range(col.ncolors):
        assert np.all(col.color[col.c[col.ptr[r]:col.ptr[r + 1]]] == r)


def test_model_equals_the_plain_python_rule(model):
    seen_unsym = 0
    for trial, n, (cp, rv, nz) in patterns():
        col = model.coloring(cp, rv)
        nc, color = python_coloring(cp, rv)
        assert col.ncolors == nc and np.array_equal(col.color, color), (trial, n)
        check_coloring(cp, rv, col)
        assert col.ncolors <= n
        S = sp.csc_matrix((np.ones(len(rv)), rv - 1, cp - 1), shape=(n, n))
        seen_unsym += (S != S.T).nnz > 0
    assert seen_unsym > 100                       # the non-symmetric patterns really are


def test_the_largest_key_is_coloured_first(model):
    """the first colour holds the vertex with the globally largest key; a vertex of colour r > 0 lost the round before its own:
    to a neighbour with a larger key that was still uncoloured then (its colour is at least r - 1)"""
    for trial, n, (cp, rv, nz) in patterns():
        col = model.coloring(cp, rv)
        N = neighbours(cp, rv)
        assert col.color[max(range(n), key=key)] == 0
        for i in range(n):
            if col.color[i] > 0:
                assert any(col.color[j] >= col.color[i] - 1 and key(j) > key(i) for j in N[i])


def test_values_do_not_influence_the_colouring(model):
    """only the pattern counts: stored 0.0, -0.0 and NaN are entries; the model's rounds take no values at all, and the reordered
    matrix moves every value's bits"""
    rng = np.random.default_rng(41)
    cp, rv, nz = random_pattern(rng, 30, False, 0.1)
    a = model.coloring(cp, rv)
    vals = rng.standard_normal(len(rv))
    vals[[0, 3, 7, 11]] = [0.0, -0.0, np.nan, np.inf]
    bcp, brv, bnz = model.reorder((cp, rv, vals), a.c)
    wcp, wrv, wnz = reorder_py((cp, rv, vals), a.c)
    assert np.array_equal(bcp, wcp) and np.array_equal(brv, wrv) and np.array_equal(bits(bnz), bits(wnz))
    assert sorted(bits(bnz).tolist()) == sorted(bits(vals).tolist())


def test_reordered_matrix_is_A_c_c(model):
    for trial, n, (cp, rv, nz) in patterns():
        if trial % 5:
            continue
        col = model.coloring(cp, rv)
        bcp, brv, bnz = model.reorder((cp, rv, nz), col.c)
        A = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).toarray()
        B = sp.csc_matrix((bnz, brv - 1, bcp - 1), shape=(n, n)).toarray()
        assert np.array_equal(B, A[np.ix_(col.c, col.c)])
        for j in range(n):
            assert np.all(np.diff(brv[bcp[j] - 1:bcp[j + 1] - 1]) > 0)


def test_every_schedule_of_the_reordered_matrix_has_at_most_ncolors_levels(model):
    """a row of colour r meets only rows of colours < r in the strictly lower part of A[c,c] and only rows of colours > r in the
    strictly upper part, so a dependency chain visits strictly increasing (decreasing) colours"""
    worst = 0
    for trial, n, (cp, rv, nz) in patterns():
        col = model.coloring(cp, rv)
        bcp, brv, _ = model.reorder((cp, rv, nz), col.c)
        for lev in level_schedules(bcp, brv):
            assert int(lev.max()) + 1 <= col.ncolors, (trial, n)
            worst = max(worst, int(lev.max()) + 1 - col.ncolors)
    assert worst == 0                             # and the bound is attained


def test_fdrand_20_cubed_needs_fewer_colours_than_levels(model, orc):
    O = orc.fdrand(20, 20, 20, style=orc.KIND_UPDATE)
    cp, rv, nz = (np.array(a) for a in O.sparse().arrays())
    natural = [int(lev.max()) + 1 for lev in level_schedules(cp, rv)]
    col = model.coloring(cp, rv)
    bcp, brv, _ = model.reorder((cp, rv, nz), col.c)
    coloured = [int(lev.max()) + 1 for lev in level_schedules(bcp, brv)]
    print("fdrand 20^3: %d colours, sizes %s; levels natural %s, coloured %s"
          % (col.ncolors, np.diff(col.ptr).tolist(), natural, coloured))
    assert natural == [58, 58, 58]
    assert col.ncolors < 58 and max(coloured) <= col.ncolors
    assert col.ncolors == 14                      # NOTES/coloring.md


def test_coloring_entry_points_declared_and_exported(esp):
    """the header declares the constant and the calls, the binding table holds them, the package exports the classes and helpers"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_COLORED\s+6\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["esp_graph_coloring", "esp_precon_colored_create", "esp_precon_colored_info", "esp_precon_colored_colors",
             "esp_precon_colored_perm", "esp_precon_colored_matrix"]
    lib = esp._lib.load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    assert esp.ESP_PRECON_COLORED == 6 and esp.ColoredPreconditioner.KIND == 6
    assert issubclass(esp.ParallelILU0Preconditioner, esp.ColoredPreconditioner)
    for name in ("graphcol", "reordermatrix", "reorderlinsys"):
        assert callable(getattr(esp, name))
    with pytest.raises(TypeError):
        esp.ColoredPreconditioner("not a matrix")
    with pytest.raises(TypeError):
        esp.graphcol("not a matrix")
