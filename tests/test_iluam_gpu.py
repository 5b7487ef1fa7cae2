"""GPU: ILUAMPreconditioner on the device CSC (include/esparse_hip.h, ESP_PRECON_ILUAM) against the independent model of
tests/iluam_model.c, which restates the reference's sequential loops (ilu_Al-Kurdi_Mittal.jl:68-187): the factorization,
ldiv! and u after any number of simple! steps are compared on bits; the level counts against a NumPy restatement of the
three schedules; the residual norms to rounding (the reference's norm is BLAS nrm2)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from iluam_modellib import Model, level_schedules
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID = -1
ESP_ERR_STATE = -6
MATRICES = ["fdrand40", "nonsymmetric", "fem2d", "diagonal", "chain"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("iluam_model"))


def host_arrays(A):
    """copies of the CSC arrays (the host copy behind A.sparse() is refreshed in place by later reads)"""
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def nonsymmetric(esp, n=3000, extra=20000, seed=5):
    """a non-symmetric matrix with a random extra pattern, every diagonal stored, built from appended triplets (a copy of
    the helper of test_precon_gpu.py); diagonally dominant, so the factorization holds no NaN -- NaN payloads need not
    agree between CPU and GPU"""
    rng = np.random.default_rng(seed)
    A = esp.ExtendableSparseMatrix(n, n)
    d = np.arange(1, n + 1)
    A.append(esp.ESP_UPDATE, d, d, 20.0 + rng.random(n))
    I = rng.integers(1, n + 1, extra)
    J = np.clip(I + rng.integers(-400, 400, extra), 1, n)
    A.append(esp.ESP_UPDATE, I, J, rng.standard_normal(extra))
    I = rng.integers(1, n + 1, 2000)
    A.append(esp.ESP_UPDATE, I, rng.integers(1, n + 1, 2000), rng.standard_normal(2000))
    A.flush()
    return A


def make_matrix(esp, name):
    if name == "fdrand40":
        return esp.fdrand(40, 40, 40, rand_mode=1, seed=11)
    if name == "nonsymmetric":
        return nonsymmetric(esp)
    if name == "fem2d":          # testassemble! on a 2-D Kuhn grid, cells in shuffled order
        npd = 64
        A = esp.ExtendableSparseMatrix(npd * npd, npd * npd)
        A.generate_fem(2, npd, seed=0x5EED0004, order_mode=1)
        A.flush()
        return A
    if name == "diagonal":       # Diagonal(1..n): one level everywhere
        n = 1000
        A = esp.ExtendableSparseMatrix(n, n)
        d = np.arange(1, n + 1)
        A.append(esp.ESP_UPDATE, d, d, d.astype(np.float64))
        A.flush()
        return A
    assert name == "chain"       # lower bidiagonal: 2000 forward levels of one row each (the thin-level path)
    n = 2000
    rng = np.random.default_rng(21)
    A = esp.ExtendableSparseMatrix(n, n)
    d = np.arange(1, n + 1)
    A.append(esp.ESP_UPDATE, d, d, 2.0 + rng.random(n))
    A.append(esp.ESP_UPDATE, d[1:], d[:-1], rng.standard_normal(n - 1))
    A.flush()
    return A


@pytest.fixture(scope="module", params=MATRICES)
def case(request, esp, model):
    """(name, A, host CSC arrays, preconditioner, the model's factorization and diag)"""
    A = make_matrix(esp, request.param)
    arrays = host_arrays(A)
    P = esp.ILUAMPreconditioner(A)
    f, diag = model.factor(arrays)
    yield request.param, A, arrays, P, f, diag
    P.close()


def assert_same(name, got, want):
    """bitwise equal.  Only the FEM matrix is not diagonally dominant: should the model's result for it hold a non-finite
    value, the finite mask and the bits of the finite entries are compared instead (NaN payloads need not agree between
    CPU and GPU)."""
    assert got.shape == want.shape
    fin = np.isfinite(want)
    if name != "fem2d":
        assert fin.all()
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(bits(got[fin]), bits(want[fin]))


def test_factor_bitwise(case):
    """1. factor() against the model's iluAM."""
    name, A, arrays, P, f, diag = case
    assert_same(name, P.factor(), f)


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("alias", [False, True])
def test_ldiv_bitwise(case, model, where, alias):
    """2. ldiv! against the model's two scatter loops, host and device vectors, x === b and not."""
    name, A, arrays, P, f, diag = case
    n = A.n
    v = np.random.default_rng(1).standard_normal(n)
    want = model.ldiv(arrays, f, diag, v)
    if where == "host":
        vv = v.copy()
        got = P.ldiv(vv, out=vv if alias else None)
        if alias:
            assert got is vv
        else:
            assert np.array_equal(vv, v)
        got = np.asarray(got)
    else:
        import torch
        tv = torch.from_numpy(v.copy()).cuda()
        got = P.ldiv(tv, out=tv if alias else None)
        if alias:
            assert got.data_ptr() == tv.data_ptr()
        else:
            assert np.array_equal(tv.cpu().numpy(), v)
        got = got.cpu().numpy()
    assert_same(name, got, want)


def test_levels(case):
    """3. levels() against the level counts a NumPy restatement computes from the pattern."""
    name, A, arrays, P, f, diag = case
    cp, rv, _ = arrays
    want = tuple(int(l.max()) + 1 for l in level_schedules(cp, rv))
    assert P.levels() == want
    if name == "fdrand40":
        assert want == (118, 118, 118)       # nx + ny + nz - 2
    if name == "diagonal":
        assert want == (1, 1, 1)
    if name == "chain":
        assert want == (1, 2000, 1)


def test_update_semantics(esp, orc, model):
    """4. the factorization owns a copy of the values (ILU0 differs here on purpose); update! with the pattern kept
    re-runs the numeric factorization on the kept analysis; the error states."""
    A = esp.fdrand(20, 20, 20, rand_mode=1, seed=3)
    cp, rv, nz0 = host_arrays(A)
    n = A.n
    P = esp.ILUAMPreconditioner(A)
    lev0 = P.levels()
    assert lev0 == (58, 58, 58)
    v = np.random.default_rng(2).standard_normal(n)
    f0, diag = model.factor((cp, rv, nz0))
    before = P.ldiv(v)
    assert np.array_equal(bits(before), bits(model.ldiv((cp, rv, nz0), f0, diag, v)))
    # a re-assembly that hits stored positions only (diagonal included): values change, the pattern stays
    rng = np.random.default_rng(4)
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    sel = rng.choice(len(rv), 5000, replace=False)
    A.append(esp.ESP_UPDATE, np.concatenate([rv[sel], np.arange(1, n + 1)]), np.concatenate([cols[sel], np.arange(1, n + 1)]),
             np.concatenate([rng.standard_normal(5000), np.full(n, 0.25)]))
    A.flush()
    cp1, rv1, nz1 = host_arrays(A)
    assert np.array_equal(cp1, cp) and np.array_equal(rv1, rv) and not np.array_equal(nz1, nz0)
    assert np.array_equal(bits(P.ldiv(v)), bits(before))            # no update!: the old factorization
    assert np.array_equal(bits(P.factor()), bits(f0))
    P.update()                                                       # values only
    f1, _ = model.factor((cp, rv, nz1))
    assert np.array_equal(bits(P.factor()), bits(f1))
    assert P.levels() == lev0
    assert np.array_equal(bits(P.ldiv(v)), bits(model.ldiv((cp, rv, nz1), f1, diag, v)))
    # pending entries -> ESP_ERR_STATE (ldiv! does not flush)
    A.append(esp.ESP_UPDATE, [1], [n], [1.0])
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    # ... flushed: a new position = a pattern change without update! -> ESP_ERR_STATE ("update! first")
    A.flush()
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    P.update()   # rebuild
    arrays2 = host_arrays(A)
    f2, diag2 = model.factor(arrays2)
    assert np.array_equal(bits(P.factor()), bits(f2))
    assert P.levels() == tuple(int(l.max()) + 1 for l in level_schedules(arrays2[0], arrays2[1]))
    assert np.array_equal(bits(P.ldiv(v)), bits(model.ldiv(arrays2, f2, diag2, v)))
    # esp_destroy refuses while a preconditioner is bound to the handle
    d = A._d
    assert d.lib.esp_destroy(d.h) == ESP_ERR_STATE
    P.close()
    assert d.lib.esp_destroy(d.h) == 0
    d.h = None


def test_errors_and_small_cases(esp):
    """4. (continued) a missing diagonal, a rectangular matrix, get_factor on another kind, n = 1."""
    B = esp.ExtendableSparseMatrix(5, 5)
    B.append(esp.ESP_UPDATE, [1, 2, 4, 5, 1], [1, 2, 4, 5, 3], [2.0, 4.0, 8.0, 16.0, 1.0])
    with pytest.raises(esp.EspError) as e:
        esp.ILUAMPreconditioner(B)
    assert e.value.code == ESP_ERR_INVALID
    J = esp.JacobiPreconditioner(B)
    buf = np.zeros(5)
    assert B._d.lib.esp_precon_get_factor(J._p, buf.ctypes.data_as(ctypes.c_void_p), 0) == ESP_ERR_INVALID
    lev = (ctypes.c_int64 * 3)(7, 7, 7)
    assert B._d.lib.esp_precon_levels(J._p, lev) == 0 and list(lev) == [0, 0, 0]
    J.close()
    d = B._d
    assert d.lib.esp_destroy(d.h) == 0   # the failed ILUAM create left nothing bound
    d.h = None
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    with pytest.raises(esp.EspError):
        esp.ILUAMPreconditioner(R)
    O = esp.ExtendableSparseMatrix(1, 1)
    O.append(esp.ESP_UPDATE, [1], [1], [4.0])
    P = esp.ILUAMPreconditioner(O)
    assert list(P.factor()) == [4.0] and P.levels() == (1, 1, 1)
    assert list(P.ldiv(np.array([8.0]))) == [2.0]
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_simple_bitwise(esp, model, where):
    """5. simple! with reltol = abstol = 0 runs all 25 steps: u bitwise equal to the model's loop, norms to rounding (the
    rtol of test_precon_gpu.py for the same residual kernel)."""
    A = esp.fdrand(30, 30, 30, rand_mode=2, seed=9)
    arrays = host_arrays(A)
    n = A.n
    f, diag = model.factor(arrays)
    rng = np.random.default_rng(6)
    b = rng.standard_normal(n)
    u0 = rng.standard_normal(n)
    P = esp.ILUAMPreconditioner(A)
    if where == "host":
        u = u0.copy()
        got, log = esp.simple(A, b, u=u, Pl=P, maxiter=25, reltol=0.0, abstol=0.0, log=True)
        assert got is u
    else:
        import torch
        tu = torch.from_numpy(u0.copy()).cuda()
        got, log = esp.simple(A, torch.from_numpy(b).cuda(), u=tu, Pl=P, maxiter=25, reltol=0.0, abstol=0.0, log=True)
        got = got.cpu().numpy()
    wu, wh, wit = model.simple(arrays, f, diag, b, u=u0, maxiter=25, abstol=0.0, reltol=0.0)
    assert wit == 25 and len(log["resnorm"]) == 26
    assert np.array_equal(bits(got), bits(wu))
    np.testing.assert_allclose(log["resnorm"], wh, rtol=1e-13, atol=0)
    P.close()


def test_simple_reference_acceptance(esp, model):
    """6. test_preconditioners.jl:10-20 with the bound line 36 puts on ILUZeroPreconditioner (the same factorization
    mathematically): simple(A, ones; Pl, maxiter = 10000, reltol = 1e-10, log = true) on fdrand(20,20,20) has a monotone
    tail, lands within 4e-5 of A \\ b, is bitwise the model's, and takes strictly fewer iterations than ILU0Preconditioner
    (the claim of ILUAMPreconditioner's docstring)."""
    A = esp.fdrand(20, 20, 20)
    arrays = host_arrays(A)
    cp, rv, nz = arrays
    n = A.n
    b = np.ones(n)
    P = esp.ILUAMPreconditioner(A)
    u, log = esp.simple(A, b, Pl=P, maxiter=10000, reltol=1e-10, log=True)
    r = log["resnorm"]
    tail = min(100, len(r) // 2)
    assert np.all(r[len(r) - 1 - tail:] / r[len(r) - 2 - tail:-1] < 1)
    exact = spla.spsolve(sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).tocsr(), b)
    err = np.linalg.norm(u - exact)
    f, diag = model.factor(arrays)
    wu, wh, wit = model.simple(arrays, f, diag, b, maxiter=10000, reltol=1e-10)
    P0 = esp.ILU0Preconditioner(A)
    _, log0 = esp.simple(A, b, Pl=P0, maxiter=10000, reltol=1e-10, log=True)
    print("iluam: %d iterations, error %.3e; ilu0: %d iterations" % (len(r) - 1, err, len(log0["resnorm"]) - 1))
    assert err <= 4e-5
    if wit != len(r) - 1:   # only a norm within rounding of the threshold may tell the two apart
        k = min(wit, len(r) - 1)
        assert abs((wh[k] / wh[0]) / 1e-10 - 1) <= 1e-12 and abs((r[k] / r[0]) / 1e-10 - 1) <= 1e-12
    else:
        assert np.array_equal(bits(u), bits(wu))
    np.testing.assert_allclose(r[:min(len(r), len(wh))], wh[:min(len(r), len(wh))], rtol=1e-12, atol=0)
    assert len(r) - 1 < len(log0["resnorm"]) - 1
    P.close()
    P0.close()


def test_full_size_256(esp, model):
    """7. 256^3: factor(), one ldiv! and 3 simple! steps bitwise equal to the model's sequential loops; 766 levels."""
    nx = 256
    A = esp.fdrand(nx, nx, nx)
    arrays = host_arrays(A)
    n = A.n
    P = esp.ILUAMPreconditioner(A)
    assert P.levels() == (766, 766, 766)
    f, diag = model.factor(arrays)
    assert np.array_equal(bits(P.factor()), bits(f))
    rng = np.random.default_rng(8)
    v = rng.standard_normal(n)
    assert np.array_equal(bits(P.ldiv(v)), bits(model.ldiv(arrays, f, diag, v)))
    b = rng.standard_normal(n)
    u, log = esp.simple(A, b, Pl=P, maxiter=3, reltol=0.0, log=True)
    wu, wh, wit = model.simple(arrays, f, diag, b, maxiter=3, reltol=0.0)
    assert wit == 3 and len(log["resnorm"]) == 4
    assert np.array_equal(bits(u), bits(wu))
    np.testing.assert_allclose(log["resnorm"], wh, rtol=1e-12, atol=0)
    P.close()
