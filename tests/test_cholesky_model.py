"""CPU: the normative model of CholeskyFactorization (tests/cholesky_model.c over lu_model.c's ordering and pattern) is
held to what the rule promises: L*L' = A[c,c], a solve as good as numpy.linalg.solve's, a pattern that contains a dense Cholesky's
fill, a strict lower triangle of A that is never read, the failing position of a dense sequential Cholesky, and an update! of the
values that equals a fresh factorization.  No GPU."""
import numpy as np
import pytest

import cholesky_modellib as CM
import lu_modellib as L
from refmodel import bits

EPS = np.finfo(np.float64).eps
GRIDS = [(5, 4, 3), (10, 10, 10), (20, 20, 1)]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return CM.Model(tmp_path_factory.mktemp("cholesky_model"))


def fdrand_csc(orc, nx, ny, nz, rand_mode=1):
    O = orc.fdrand(nx, ny, nz, rand_mode=rand_mode, style=orc.KIND_UPDATE)
    return tuple(np.array(a) for a in O.sparse().arrays())


_facts = {}


def fact_of(model, orc, grid):
    """one factorization per grid, shared and left unchanged"""
    if grid not in _facts:
        csc = fdrand_csc(orc, *grid)
        _facts[grid] = (csc, model.cholesky(csc, 16))
    return _facts[grid]


@pytest.mark.parametrize("grid", GRIDS)
def test_factor_reproduces_the_matrix(model, orc, grid):
    csc, F = fact_of(model, orc, grid)
    S = CM.symmetric_dense(csc)[np.ix_(F.c, F.c)]
    Lm = F.dense_L()
    # every entry of L*L' is a sum of at most n rounded products of entries bounded through |l_ik| <= sqrt(a_ii): the bound scales
    # with sqrt(a_ii * a_jj)
    scale = np.sqrt(np.outer(np.diag(S), np.diag(S)))
    err = np.abs(Lm @ Lm.T - S) / scale
    print("grid %s: max scaled |L*L' - A[c,c]| = %.3g eps" % (grid, err.max() / EPS))
    assert err.max() <= 64 * EPS


@pytest.mark.parametrize("grid", GRIDS)
def test_solve_residual(model, orc, grid):
    csc, F = fact_of(model, orc, grid)
    S = CM.symmetric_dense(csc)
    b = np.random.default_rng(5).standard_normal(F.n)
    x = F.solve(b)
    r = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    r_np = np.linalg.norm(b - S @ np.linalg.solve(S, b)) / np.linalg.norm(b)
    print("grid %s: residual model %.3e, numpy.linalg.solve %.3e" % (grid, r, r_np))
    assert r <= 16 * r_np
    y = b.copy()
    assert F.ldiv(y, inplace=True) is y and np.array_equal(bits(y), bits(x))


@pytest.mark.parametrize("grid", GRIDS)
def test_pattern_contains_the_dense_fill(model, orc, grid):
    csc, F = fact_of(model, orc, grid)
    S = CM.symmetric_dense(csc)[np.ix_(F.c, F.c)]
    P = L.pattern_of(F.lcp, F.lrv)
    assert not np.triu(P, 1).any()
    assert not (np.linalg.cholesky(S) != 0.0)[~P].any()
    assert P[np.tril(S) != 0.0].all()


def test_strict_lower_triangle_is_never_read(model, orc):
    csc, F = fact_of(model, orc, (5, 4, 3))
    cp, rv, nz = (a.copy() for a in csc)
    col = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
    lower = rv - 1 > col
    assert lower.any()
    nz[lower] = np.where(np.arange(lower.sum()) % 2 == 0, np.nan, -1e300)
    G = model.cholesky((cp, rv, nz), 16)
    assert np.array_equal(G.lrv, F.lrv) and np.array_equal(bits(G.L[2]), bits(F.L[2]))


def indefinite(orc, how):
    cp, rv, nz = fdrand_csc(orc, 6, 5, 1)
    col = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
    d = int(np.flatnonzero((rv - 1 == col) & (col == 17))[0])
    if how == "negated":
        nz = nz.copy()
        nz[d] = -nz[d]
        return cp, rv, nz
    cp = cp.copy()
    cp[18:] -= 1
    return cp, np.delete(rv, d), np.delete(nz, d)


@pytest.mark.parametrize("how", ["negated", "removed"])
def test_failing_position_is_the_dense_one(model, orc, how):
    csc = indefinite(orc, how)
    good = model.cholesky(fdrand_csc(orc, 6, 5, 1), 4)
    with pytest.raises(CM.NotPosDef) as e:
        model.cholesky(csc, 4)
    c = good.c                                                     # (the removed diagonal takes no part in the graph: the same order)
    S = CM.symmetric_dense(csc)[np.ix_(c, c)]
    want = CM.dense_cholesky_position(S)
    assert want >= 0 and e.value.position == want and e.value.column == c[want]


def test_values_only_update_equals_fresh(model, orc):
    csc = fdrand_csc(orc, 5, 4, 3)
    other = fdrand_csc(orc, 5, 4, 3, rand_mode=2)
    assert np.array_equal(csc[1], other[1]) and not np.array_equal(csc[2], other[2])
    F = model.cholesky(csc, 16)
    F.update(other)
    G = model.cholesky(other, 16)
    assert F.builds == 1
    assert np.array_equal(bits(F.L[2]), bits(G.L[2]))
    b = np.arange(1.0, F.n + 1)
    assert np.array_equal(bits(F.solve(b)), bits(G.solve(b)))


def test_model_main_under_sanitizers(tmp_path):
    """tests/cholesky_model_main.c, a stand-alone program over the model, built with AddressSanitizer and UBSan and run on the CPU"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "cholesky_model_main")
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(here, "cholesky_model_main.c"), os.path.join(here, "cholesky_model.c"), "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cholesky_model_main: ok" in r.stdout, (r.stdout, r.stderr)
