"""GPU: the point preconditioners' update! / ldiv! and simple! on the device CSC (include/esparse_hip.h, esp_precon_*,
esp_simple) against the independent model of tests/precon_model.c -- bitwise for ldiv! and for u after any number of
simple! steps; the residual norms to rounding (the reference's norm is BLAS nrm2)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from precon_modellib import KIND_ILU0, KIND_JACOBI, Model
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_STATE = -6
KINDS = {"jacobi": KIND_JACOBI, "ilu0": KIND_ILU0}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("precon_model"))


def host_arrays(A):
    """copies of the CSC arrays (the host copy behind A.sparse() is refreshed in place by later reads)"""
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def make_precon(esp, A, kind):
    return esp.JacobiPreconditioner(A) if kind == "jacobi" else esp.ILU0Preconditioner(A)


def model_ldiv(model, orc, kind, arrays, v):
    """ldiv! of the reference with the factorization of `arrays` (an oracle CSC built from them)"""
    cp, rv, nz = arrays
    n = len(cp) - 1
    C = orc.CSC(n, n, cp, rv, nz)
    if kind == "jacobi":
        return model.jacobi_ldiv(C.jacobi(), v)
    xd, idg = C.ilu0()
    return model.ilu0_ldiv(arrays, xd, idg, v)


def nonsymmetric(esp, n=3000, extra=20000, seed=5):
    """a non-symmetric matrix with a random extra pattern, every diagonal stored, built from appended triplets"""
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


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
@pytest.mark.parametrize("matrix", ["fdrand40", "nonsymmetric"])
@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("alias", [False, True])
def test_ldiv_bitwise(esp, orc, model, kind, matrix, where, alias):
    if matrix == "fdrand40":
        A = esp.fdrand(40, 40, 40, rand_mode=1, seed=11)
        O = orc.fdrand(40, 40, 40, rand_mode=1, seed=11, style=orc.KIND_UPDATE)
        arrays = O.sparse().arrays()
        for got, want in zip(host_arrays(A), arrays):
            assert np.array_equal(bits(got) if got.dtype == np.float64 else got, bits(want) if want.dtype == np.float64 else want)
    else:
        A = nonsymmetric(esp)
        arrays = host_arrays(A)
    n = A.n
    v = np.random.default_rng(1).standard_normal(n)
    want = model_ldiv(model, orc, kind, arrays, v)
    P = make_precon(esp, A, kind)
    if where == "host":
        vv = v.copy()
        got = P.ldiv(vv, out=vv if alias else None)
        if alias:
            assert got is vv
        got = np.asarray(got)
    else:
        import torch
        tv = torch.from_numpy(v.copy()).cuda()
        got = P.ldiv(tv, out=tv if alias else None)
        if alias:
            assert got.data_ptr() == tv.data_ptr()
        got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    P.close()


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
def test_update_semantics(esp, orc, model, kind):
    """update! (jacobi.jl:54-64, ilu0.jl:120-130) and ldiv! between updates: the reference's preconditioner holds
    A.cscmatrix by reference, so a same-pattern re-assembly without update! gives the CURRENT nzval with the OLD diagonal."""
    A = esp.fdrand(20, 20, 20, rand_mode=1, seed=3)
    cp, rv, nz0 = host_arrays(A)
    n = A.n
    C_old = orc.CSC(n, n, cp, rv, nz0)
    P = make_precon(esp, A, kind)
    v = np.random.default_rng(2).standard_normal(n)
    # a re-assembly that hits stored positions only (diagonal included): values change, the pattern stays
    rng = np.random.default_rng(4)
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    sel = rng.choice(len(rv), 5000, replace=False)
    A.append(esp.ESP_UPDATE, np.concatenate([rv[sel], np.arange(1, n + 1)]), np.concatenate([cols[sel], np.arange(1, n + 1)]),
             np.concatenate([rng.standard_normal(5000), np.full(n, 0.25)]))
    A.flush()
    cp1, rv1, nz1 = host_arrays(A)
    assert np.array_equal(cp1, cp) and np.array_equal(rv1, rv) and not np.array_equal(nz1, nz0)
    got = P.ldiv(v)
    if kind == "jacobi":
        want = model.jacobi_ldiv(C_old.jacobi(), v)
    else:
        xd_old, idg = C_old.ilu0()
        want = model.ilu0_ldiv((cp, rv, nz1), xd_old, idg, v)   # new nzval, old xdiag
    assert np.array_equal(bits(got), bits(want))
    # eliminate_dirichlet! edits values in place too
    mk = np.zeros(n, bool)
    mk[::97] = True
    A.eliminate_dirichlet(mk)
    cp2, rv2, nz2 = host_arrays(A)
    got = P.ldiv(v)
    if kind == "ilu0":
        assert np.array_equal(bits(got), bits(model.ilu0_ldiv((cp, rv, nz2), xd_old, idg, v)))
    else:
        assert np.array_equal(bits(got), bits(want))
    # update!: values only -> the new factorization
    P.update()
    assert np.array_equal(bits(P.ldiv(v)), bits(model_ldiv(model, orc, kind, (cp2, rv2, nz2), v)))
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
    assert np.array_equal(bits(P.ldiv(v)), bits(model_ldiv(model, orc, kind, host_arrays(A), v)))
    # esp_destroy refuses while a preconditioner is bound to the handle
    d = A._d
    assert d.lib.esp_destroy(d.h) == ESP_ERR_STATE
    P.close()
    assert d.lib.esp_destroy(d.h) == 0
    d.h = None


def test_missing_diagonal_and_rectangular(esp):
    B = esp.ExtendableSparseMatrix(5, 5)
    B.append(esp.ESP_UPDATE, [1, 2, 4, 5, 1], [1, 2, 4, 5, 3], [2.0, 4.0, 8.0, 16.0, 1.0])
    with pytest.raises(esp.EspError):
        esp.ILU0Preconditioner(B)
    J = esp.JacobiPreconditioner(B)
    u = J.ldiv(np.ones(5))
    assert list(u[[0, 1, 3, 4]]) == [0.5, 0.25, 0.125, 0.0625] and np.isinf(u[2])
    J.close()
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    for cls in (esp.JacobiPreconditioner, esp.ILU0Preconditioner):
        with pytest.raises(esp.EspError):
            cls(R)
    d = B._d
    assert d.lib.esp_destroy(d.h) == 0   # the failed ILU0 create left nothing bound
    d.h = None


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_simple_bitwise(esp, orc, model, kind, where):
    """simple! with reltol = abstol = 0 runs all maxiter steps: u bitwise equal to the model's loop, norms to rounding."""
    A = esp.fdrand(30, 30, 30, rand_mode=2, seed=9)
    arrays = host_arrays(A)
    cp, rv, nz = arrays
    n = A.n
    C = orc.CSC(n, n, cp, rv, nz)
    diag, idg = (C.jacobi(), None) if kind == "jacobi" else C.ilu0()
    rng = np.random.default_rng(6)
    b = rng.standard_normal(n)
    u0 = rng.standard_normal(n)
    P = make_precon(esp, A, kind)
    if where == "host":
        u = u0.copy()
        got, log = esp.simple(A, b, u=u, Pl=P, maxiter=25, reltol=0.0, abstol=0.0, log=True)
        assert got is u
    else:
        import torch
        tu = torch.from_numpy(u0.copy()).cuda()
        got, log = esp.simple(A, torch.from_numpy(b).cuda(), u=tu, Pl=P, maxiter=25, reltol=0.0, abstol=0.0, log=True)
        got = got.cpu().numpy()
    wu, wh, wit = model.simple(KINDS[kind], arrays, diag, idg, b, u=u0, maxiter=25, abstol=0.0, reltol=0.0)
    assert wit == 25 and len(log["resnorm"]) == 26
    assert np.array_equal(bits(got), bits(wu))
    np.testing.assert_allclose(log["resnorm"], wh, rtol=1e-13, atol=0)
    P.close()


@pytest.mark.parametrize("kind,bound", [("ilu0", 4e-5), ("jacobi", 3e-4)])
def test_simple_reference_acceptance(esp, orc, model, kind, bound):
    """test_preconditioners.jl:34-36 on the device: simple(A, ones; Pl, maxiter = 10000, reltol = 1e-10, log = true) on
    fdrand(20,20,20): monotone tail, within 4e-5 (ILU0) / 3e-4 (Jacobi) of A \\ b, u bitwise the model's."""
    A = esp.fdrand(20, 20, 20)
    arrays = host_arrays(A)
    cp, rv, nz = arrays
    n = A.n
    b = np.ones(n)
    P = make_precon(esp, A, kind)
    u, log = esp.simple(A, b, Pl=P, maxiter=10000, reltol=1e-10, log=True)
    r = log["resnorm"]
    tail = min(100, len(r) // 2)
    assert np.all(r[len(r) - 1 - tail:] / r[len(r) - 2 - tail:-1] < 1)
    exact = spla.spsolve(sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).tocsr(), b)
    assert np.linalg.norm(u - exact) <= bound
    C = orc.CSC(n, n, cp, rv, nz)
    diag, idg = (C.jacobi(), None) if kind == "jacobi" else C.ilu0()
    wu, wh, wit = model.simple(KINDS[kind], arrays, diag, idg, b, maxiter=10000, reltol=1e-10)
    if wit != len(r) - 1:   # only a norm within rounding of the threshold may tell the two apart
        k = min(wit, len(r) - 1)
        assert abs((wh[k] / wh[0]) / 1e-10 - 1) <= 1e-12 and abs((r[k] / r[0]) / 1e-10 - 1) <= 1e-12
    else:
        assert np.array_equal(bits(u), bits(wu))
    np.testing.assert_allclose(r[:min(len(r), len(wh))], wh[:min(len(r), len(wh))], rtol=1e-12, atol=0)
    P.close()


def test_full_size_256(esp, model):
    """256^3: one ILU0 ldiv! and 5 simple! steps bitwise equal to the model's column loops."""
    nx = 256
    A = esp.fdrand(nx, nx, nx)
    arrays = host_arrays(A)
    n = A.n
    xd, idg = A.ilu0()      # (bit-identical to the oracle's ilu0: test_gpu_parity.py::test_jacobi_and_ilu0_setup)
    P = esp.ILU0Preconditioner(A)
    rng = np.random.default_rng(8)
    v = rng.standard_normal(n)
    assert np.array_equal(bits(P.ldiv(v)), bits(model.ilu0_ldiv(arrays, xd, idg, v)))
    b = rng.standard_normal(n)
    u, log = esp.simple(A, b, Pl=P, maxiter=5, reltol=0.0, log=True)
    wu, wh, wit = model.simple(KIND_ILU0, arrays, xd, idg, b, maxiter=5, reltol=0.0)
    assert wit == 5 and len(log["resnorm"]) == 6
    assert np.array_equal(bits(u), bits(wu))
    np.testing.assert_allclose(log["resnorm"], wh, rtol=1e-12, atol=0)
    P.close()
