"""CPU: the independent model of ILUKPreconditioner's filled matrix (tests/iluk_model.c, the sequential level-of-fill rule) is held
to account -- against an exhaustive fill-path enumeration, against the parallel form the device uses (one bounded search per
column, tests/iluk_modellib.py), on the cases where the answer is known (K = 0, no fill at all, complete fill = LU) -- and the
new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from iluk_modellib import Model, fill_path_levels, levels_as_dict, parallel_levels
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("iluk_model"))


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


def check_values(csc, B, lev):
    """A's bits where the level is 0, +0.0 elsewhere; level 0 exactly on A's positions"""
    cp, rv, nz = csc
    bcp, brv, bnz = B
    have = {(int(rv[q]) - 1, j): q for j in range(len(cp) - 1) for q in range(cp[j] - 1, cp[j + 1] - 1)}
    zero = 0
    for j in range(len(bcp) - 1):
        rows = brv[bcp[j] - 1:bcp[j + 1] - 1]
        assert np.all(np.diff(rows) > 0)
        for q in range(bcp[j] - 1, bcp[j + 1] - 1):
            key = (int(brv[q]) - 1, j)
            if lev[q] == 0:
                zero += 1
                assert bits(bnz[q:q + 1])[0] == bits(nz[have[key]:have[key] + 1])[0]
            else:
                assert key not in have and bits(bnz[q:q + 1])[0] == 0
    assert zero == len(rv)


def test_model_equals_fill_path_enumeration(model):
    """lev(i,j) + 1 is the length of the shortest path i -> j through vertices below min(i,j): every simple path is walked"""
    rng = np.random.default_rng(20)
    for trial in range(60):
        n = int(rng.integers(1, 11))
        csc = random_pattern(rng, n, trial % 2 == 0, rng.choice([0.12, 0.25, 0.4]))
        for K in (0, 1, 2, 3, n):
            B, lev = model.fill(csc, K)
            assert levels_as_dict(B, lev) == fill_path_levels(csc[0], csc[1], K), (trial, n, K)
            check_values(csc, B, lev)


def test_parallel_form_equals_model(model):
    """the bounded search per column over A and over transpose(A) gives the sequential rule's pattern and levels"""
    rng = np.random.default_rng(21)
    for trial in range(300):
        n = int(rng.integers(3, 17))
        csc = random_pattern(rng, n, trial % 2 == 0, rng.choice([0.08, 0.15, 0.3]))
        for K in (0, 1, 2, 3, n):
            B, lev = model.fill(csc, K)
            got, vl, vu = parallel_levels(csc[0], csc[1], K)
            assert got == levels_as_dict(B, lev), (trial, n, K)
            assert max(vl) <= n and max(vu) <= n


def test_k0_is_the_matrix_itself(model):
    rng = np.random.default_rng(22)
    cp, rv, nz = random_pattern(rng, 30, False, 0.1)
    nz = rng.standard_normal(len(rv))
    nz[[1, 5, 9]] = [0.0, -0.0, np.nan]             # stored is stored: structure alone decides
    (bcp, brv, bnz), lev = model.fill((cp, rv, nz), 0)
    assert np.array_equal(bcp, cp) and np.array_equal(brv, rv) and np.array_equal(bits(bnz), bits(nz)) and not lev.any()


@pytest.mark.parametrize("which", ["tridiagonal", "diagonal"])
def test_no_fill_at_any_level(model, which):
    n = 12
    S = sp.diags([-1.0 * np.ones(n - 1), 4.0 * np.ones(n), -2.0 * np.ones(n - 1)], [-1, 0, 1]) if which == "tridiagonal" \
        else sp.diags([3.0 * np.ones(n)], [0])
    csc = csc_of(S)
    for K in (0, 1, 2, 3, n):
        (bcp, brv, bnz), lev = model.fill(csc, K)
        assert np.array_equal(bcp, csc[0]) and np.array_equal(brv, csc[1]) and np.array_equal(bits(bnz), bits(csc[2]))
        assert not lev.any()


def dominant_nonsymmetric(n=60, seed=31):
    """a seeded strictly diagonally dominant (by columns and by rows) non-symmetric matrix"""
    rng = np.random.default_rng(seed)
    M = np.where(rng.random((n, n)) < 0.08, rng.standard_normal((n, n)), 0.0)
    np.fill_diagonal(M, 0.0)
    M[np.arange(1, n), np.arange(n - 1)] = -1.0     # irreducible
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    return csc_of(sp.csc_matrix(M))


@pytest.mark.parametrize("which", ["fdrand", "dominant"])
def test_complete_fill_is_a_direct_solve(model, orc, which):
    """K = n: the pattern is closed (K + 1 adds nothing), ILU(K) is LU without pivoting, and ldiv! solves the system: the relative
    residual is at most 16 times numpy.linalg.solve's (another elimination order; the growth factor of a diagonally dominant
    matrix is at most 2)"""
    if which == "fdrand":
        O = orc.fdrand(5, 4, 3, style=orc.KIND_UPDATE)
        csc = tuple(np.array(a) for a in O.sparse().arrays())
    else:
        csc = dominant_nonsymmetric()
    n = len(csc[0]) - 1
    P = model.precon(csc, n)
    B1, lev1 = model.fill(csc, n + 1)
    assert np.array_equal(B1[0], P.B[0]) and np.array_equal(B1[1], P.B[1]) and np.array_equal(lev1, P.lev)
    assert P.lev.max() <= n - 2
    A = sp.csc_matrix((csc[2], csc[1] - 1, csc[0] - 1), shape=(n, n)).toarray()
    b = np.random.default_rng(5).standard_normal(n)
    x = P.ldiv(b)
    ref = np.linalg.solve(A, b)
    r = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    r_ref = np.linalg.norm(b - A @ ref) / np.linalg.norm(b)
    print("complete fill %s: n = %d, nnz(B) = %d of %d, |b - A x|/|b| = %.3e, numpy.linalg.solve %.3e"
          % (which, n, len(P.B[1]), len(csc[1]), r, r_ref))
    assert r <= 16 * r_ref
    assert np.array_equal(bits(P.ldiv(b, inplace=True)), bits(x))


def test_a_missing_diagonal_is_refused(model):
    """the preconditioner is ILUAM of B: a column of A without a stored diagonal is ILUAM's error (the searches never emit a diagonal)"""
    csc = csc_of(sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))
    got, _, _ = parallel_levels(csc[0], csc[1], 2)
    assert (2, 2) not in got
    with pytest.raises(ValueError):
        model.precon(csc, 2)


def test_iluk_entry_points_declared_and_exported(esp):
    """the header declares the constants and the four calls, the binding table holds them, the package exports the class"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_ILUK\s+5\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["esp_precon_iluk_create", "esp_precon_iluk_matrix", "esp_precon_iluk_levels", "esp_precon_iluk_stats"]
    lib = esp._lib.load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    for name in ("ESP_ILUK_WAVE_VISITS", "ESP_ILUK_VISIT_MAX"):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
        assert m and int(m.group(1)) == getattr(esp._lib, name)
    assert esp._lib.ESP_ILUK_WAVE_VISITS < esp._lib.ESP_ILUK_VISIT_MAX
    assert esp.ESP_PRECON_ILUK == 5 and esp.ILUKPreconditioner.KIND == 5
    with pytest.raises(TypeError):
        esp.ILUKPreconditioner("not a matrix")
