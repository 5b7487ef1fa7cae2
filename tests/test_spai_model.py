"""CPU: the normative model of SPAIPreconditioner (tests/spai_model.c) is held to account -- against numpy.linalg.lstsq column by
column, on the local problem sizes it reports, on the symmetrised form and on what the preconditioner is for: fewer cg iterations
than Jacobi -- and the new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from refmodel import bits
from spai_modellib import (JacobiPrecon, Model, SolverModel, csc_from_columns, hub_columns, sized_columns, too_large_columns,
                           transpose)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("spai_model"))


def csc_of(S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def dense_of(csc):
    cp, rv, nz = csc
    n = len(cp) - 1
    return sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).toarray()


def dominant(rng, n, symmetric_pattern, density):
    """a seeded strictly diagonally dominant matrix (by columns and by rows) on a random pattern with a full diagonal"""
    mask = rng.random((n, n)) < density
    if symmetric_pattern:
        mask = mask | mask.T
    M = np.where(mask, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    np.fill_diagonal(M, 0.0)
    keep = mask & ~np.eye(n, dtype=bool)
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    S = sp.csc_matrix(M)
    # (an off-diagonal draw is never exactly zero: the stored pattern is the mask)
    assert S.nnz == keep.sum() + n
    return csc_of(S)


def lstsq_column(csc, k):
    """column k of M by numpy.linalg.lstsq on the same I and J"""
    cp, rv, nz = csc
    A = dense_of(csc)
    J = rv[cp[k] - 1:cp[k + 1] - 1] - 1
    I = sorted(set(int(r) - 1 for j in J for r in rv[cp[j] - 1:cp[j + 1] - 1]))
    e = np.array([1.0 if i == k else 0.0 for i in I])
    return np.linalg.lstsq(A[np.ix_(I, J)], e, rcond=None)[0], len(I), len(J)


def test_model_against_lstsq(model):
    """320 seeded diagonally dominant matrices, n <= 40, symmetric and unsymmetric patterns: every column of M within
    1e-10 * max(1, |m_ref|_inf) of numpy.linalg.lstsq on the same local problem; p of every column is the size of its row set"""
    rng = np.random.default_rng(70)
    worst = 0.0
    for trial in range(320):
        n = int(rng.integers(1, 41))
        csc = dominant(rng, n, trial % 2 == 0, rng.choice([0.05, 0.1, 0.2]))
        m, pcol, stats = model.spai1(csc)
        cp = csc[0]
        mp = mq = 0
        for k in range(n):
            ref, p, q = lstsq_column(csc, k)
            got = m[cp[k] - 1:cp[k + 1] - 1]
            err = np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(ref)))
            worst = max(worst, err)
            assert err <= 1e-10, (trial, n, k, err)
            assert pcol[k] == p
            mp, mq = max(mp, p), max(mq, q)
        assert stats[0] == mp and stats[1] == mq
    print("largest |m - m_lstsq|_inf / max(1, |m_lstsq|_inf) over 320 matrices: %.3e" % worst)


def test_spai0_is_the_one_line_rule(model):
    rng = np.random.default_rng(71)
    csc = dominant(rng, 30, False, 0.2)
    A = dense_of(csc)
    d = model.spai0(csc)
    assert np.allclose(d, np.diag(A) / (A * A).sum(0), rtol=1e-14, atol=0.0)
    cols = [[0, 1], [0], []]                       # no stored diagonal in column 1; an empty column
    csc = csc_from_columns(cols, rng)
    d = model.spai0(csc)
    assert d[0] != 0.0 and bits(d[1:2])[0] == 0 and np.isnan(d[2])


def test_stencil_problem_sizes(model, orc):
    """the 7-point stencil's largest local problem is 25 x 7: the wave tier's"""
    O = orc.fdrand(5, 5, 5, style=orc.KIND_UPDATE)
    csc = tuple(np.array(a) for a in O.sparse().arrays())
    _, pcol, stats = model.spai1(csc)
    assert stats == (25, 7, 175) and pcol.max() == 25 and pcol[62] == 25      # (the centre of the grid)


def test_constructed_columns_have_the_sizes_the_gpu_tests_rely_on(model, esp):
    rng = np.random.default_rng(72)
    W, D = esp._lib.ESP_SPAI_WAVE_DOUBLES, esp._lib.ESP_SPAI_DENSE_MAX
    assert W == 64 * 8 and W + 1 == 57 * 9
    for p, q in ((64, 8), (57, 9)):
        csc = csc_from_columns(sized_columns(p, q), rng)
        _, pcol, stats = model.spai1(csc)
        assert pcol[0] == p and csc[0][1] - csc[0][0] == q and stats[2] == p * q
    for h in (63, 64, 65, 130):
        csc = csc_from_columns(hub_columns(h), rng)
        m, pcol, stats = model.spai1(csc)
        assert pcol[1] == h + 1 and pcol[0] == 3 and stats == (h + 1, h, 3 * (h + 1))
        assert np.all(np.isfinite(m[csc[0][1] - 1:csc[0][2] - 1]))
    assert D + 1 == 12289
    cp, rv, _ = csc_from_columns(too_large_columns(D + 1), rng)
    assert cp[1] - cp[0] == 1 and cp[2] - cp[1] == D + 1


def test_rank_deficient_and_degenerate_columns(model):
    """two identical columns make the local problems that hold both rank-deficient: a zero pivot is no error, NaN and Inf
    propagate; a column without a stored diagonal and an empty column are valid"""
    A = np.array([[4.0, 0.0, 0.0, 0.0],
                  [0.0, 2.0, 2.0, 1.0],
                  [0.0, 0.0, 0.0, 1.0],
                  [0.0, 0.0, 0.0, 0.0]])
    csc = csc_of(sp.csc_matrix(A))
    with np.errstate(all="ignore"):
        m, pcol, _ = model.spai1(csc)
    # column 3 holds the columns 1 and 2, both 2*e_1: B = [2 2], the second pivot is exactly zero, and p = 1 < q = 2
    assert pcol[3] == 1 and np.all(np.isnan(m[csc[0][3] - 1:csc[0][4] - 1]))
    assert m[0] == 0.25 and m[1] == 0.5                                   # columns 0 and 1 hold themselves alone
    rng = np.random.default_rng(73)
    csc = csc_from_columns([[0, 1], [0, 2], [], [3]], rng)
    with np.errstate(all="ignore"):
        m, pcol, _ = model.spai1(csc)
    assert list(pcol) == [3, 2, 0, 1] and len(m) == 5


def test_symmetrised_m_is_bitwise_symmetric(model, orc):
    O = orc.fdrand(4, 3, 3, style=orc.KIND_UPDATE)
    csc = tuple(np.array(a) for a in O.sparse().arrays())
    assert np.array_equal(dense_of(csc), dense_of(csc).T)
    P = model.precon(csc, 1, True)
    tcp, trv, tnz = transpose(P.M)
    assert np.array_equal(tcp, P.M[0]) and np.array_equal(trv, P.M[1]) and np.array_equal(bits(tnz), bits(P.M[2]))
    raw_t = transpose(P.raw)
    assert not np.array_equal(bits(raw_t[2]), bits(P.raw[2]))              # (the raw M is not symmetric: the test means something)
    assert np.all(np.linalg.eigvalsh(dense_of(P.M)) > 0)


def test_symmetrised_spai1_beats_jacobi_in_cg(model, orc):
    """fdrand 8^3, b = A*ones, rtol 1e-8, the statement-by-statement cg model: fewer iterations than Jacobi; SPAI-0 stays with
    Jacobi"""
    O = orc.fdrand(8, 8, 8, style=orc.KIND_UPDATE)
    csc = tuple(np.array(a) for a in O.sparse().arrays())
    n = len(csc[0]) - 1
    b = model.solver.mul(csc, np.ones(n))
    iters = {}
    for name, P in (("jacobi", JacobiPrecon(csc)), ("spai0", model.precon(csc, 0)), ("spai1sym", model.precon(csc, 1, True))):
        x, hist, it, conv = SolverModel(model.solver, P).cg(b, reltol=1e-8)
        assert conv and np.linalg.norm(x - 1.0) <= 1e-6 * np.sqrt(n)
        iters[name] = it
    print("cg iterations on fdrand 8^3 to 1e-8:", iters)
    assert iters["spai1sym"] < iters["jacobi"]
    assert abs(iters["spai0"] - iters["jacobi"]) <= iters["jacobi"] // 4


def test_spai_entry_points_declared_and_exported(esp):
    """the header declares the constants and the three calls, the binding table holds them, the package exports the classes"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_SPAI\s+7\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = esp._lib.load()
    for name in ("esp_precon_spai_create", "esp_precon_spai_matrix", "esp_precon_spai_stats"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    for name in ("ESP_SPAI_WAVE_DOUBLES", "ESP_SPAI_DENSE_MAX"):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
        assert m and int(m.group(1)) == getattr(esp._lib, name)
    assert 25 * 7 <= esp._lib.ESP_SPAI_WAVE_DOUBLES < esp._lib.ESP_SPAI_DENSE_MAX == 12288
    assert esp.ESP_PRECON_SPAI == 7 == esp.SPAIPreconditioner.KIND
    with pytest.raises(TypeError):
        esp.SPAIPreconditioner("not a matrix")
    with pytest.raises(NotImplementedError) as e:
        esp.AMGCL_RLXPreconditioner("not a matrix", type="ilu0")
    assert "spai0" in str(e.value) and "spai1" in str(e.value)
