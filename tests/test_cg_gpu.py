"""GPU: preconditioned conjugate gradients on the device CSC (include/esparse_hip.h, esp_cg; cg of the package) against the
model of tests/cg_model.c -- x AND the whole residual history bit for bit: ldiv! and mul! are the reference's literal loops
there, the dot products the device's fixed summation shape restated on its own."""
import ctypes
import math

import numpy as np
import pytest

from cg_modellib import KIND_ILU0, KIND_JACOBI, RELTOL, Model, Precon
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_STATE = -1, -6
KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("cg_model"))


def host_arrays(A):
    """copies of the CSC arrays (the host copy behind A.sparse() is refreshed in place by later reads)"""
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def make_precon(esp, A, kind):
    return {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
            "iluam": esp.ILUAMPreconditioner}[kind](A)


def close(P):
    if P is not None:
        P.close()


def isapprox(x, y):
    """Julia's x ≈ y for vectors: norm(x - y) <= sqrt(eps) * max(norm(x), norm(y))"""
    return np.linalg.norm(x - y) <= math.sqrt(EPS) * max(np.linalg.norm(x), np.linalg.norm(y))


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN (its payload is the hardware's business), at the same positions only"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


MATRICES = {"fdrand20": (20, 20, 20), "fdrand40": (40, 40, 40), "fdrand100x100": (100, 100, 1)}


def oracle_matrix(esp, orc, name):
    """the matrix on the device, its CSC held bitwise to the oracle's"""
    dims = MATRICES[name]
    A = esp.fdrand(*dims)
    O = orc.fdrand(*dims, style=orc.KIND_UPDATE)
    arrays = host_arrays(A)
    for got, want in zip(arrays, O.sparse().arrays()):
        assert np.array_equal(bits(got) if got.dtype == np.float64 else got, bits(want) if want.dtype == np.float64 else want)
    return A, arrays


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


def run_device(esp, A, b, P, where, x0=None, **kw):
    """cg (x0 None) or cg! on host arrays or torch tensors -> (x as a NumPy array, log)"""
    if where == "host":
        x = None if x0 is None else x0.copy()
        got, log = esp.cg(A, b, Pl=P, x=x, log=True, **kw)
        if x is not None:
            assert got is x
        return np.asarray(got), log
    import torch
    tx = None if x0 is None else torch.from_numpy(x0.copy()).cuda()
    got, log = esp.cg(A, torch.from_numpy(np.ascontiguousarray(b)).cuda(), Pl=P, x=tx, log=True, **kw)
    if tx is not None:
        assert got.data_ptr() == tx.data_ptr()
    return got.cpu().numpy(), log


def check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=None, **kw):
    P = make_precon(esp, A, kind)
    try:
        got, log = run_device(esp, A, b, P, where, x0=x0, **kw)
        wx, wh, wit, wconv = model.cg(model.precon(kind, arrays, orc), arrays, b, x=x0, **kw)
        print("%s %s: %d iterations (model %d), converged %s, last norm %.3e"
              % (kind, where, log["iters"], wit, log["isconverged"], history_of(log)[-1]))
        assert log["iters"] == wit and log["isconverged"] == wconv and len(log["resnorm"]) == wit
        assert same_bits(history_of(log), wh)
        assert same_bits(got, wx)
        return got, log
    finally:
        close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("matrix", ["fdrand20", "fdrand40", "fdrand100x100"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg_bitwise(esp, orc, model, kind, matrix, where):
    """cg(A, b; Pl) with b = A*ones to the default tolerance: x and the history bit for bit the model's"""
    A, arrays = oracle_matrix(esp, orc, matrix)
    b = model.mul(arrays, np.ones(A.n))
    check_against_model(model, orc, esp, A, arrays, kind, b, where)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg_inplace_from_a_random_start(esp, orc, model, kind, where):
    """cg!(x, A, b; Pl): r = b - A*x first, x updated in place"""
    A, arrays = oracle_matrix(esp, orc, "fdrand20")
    rng = np.random.default_rng(21)
    b = rng.standard_normal(A.n)
    check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=rng.standard_normal(A.n))


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("maxiter", [1, 2, 7])
def test_truncation(esp, orc, model, kind, maxiter):
    """maxiter cuts the loop: bitwise after k iterations, not converged"""
    A, arrays = oracle_matrix(esp, orc, "fdrand20")
    b = model.mul(arrays, np.ones(A.n))
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", maxiter=maxiter)
    assert log["iters"] == maxiter and not log["isconverged"]


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_two_runs_identical(esp, orc, kind):
    A, _ = oracle_matrix(esp, orc, "fdrand40")
    b = np.random.default_rng(4).standard_normal(A.n)
    P = make_precon(esp, A, kind)
    x1, l1 = run_device(esp, A, b, P, "torch", maxiter=60)
    x2, l2 = run_device(esp, A, b, P, "torch", maxiter=60)
    assert same_bits(x1, x2) and same_bits(history_of(l1), history_of(l2)) and l1["iters"] == l2["iters"] > 0
    close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_zero_right_hand_side(esp, orc, kind, where):
    """b = 0: residual 0 <= tol 0 -- no iteration, x untouched, converged"""
    A, _ = oracle_matrix(esp, orc, "fdrand20")
    P = make_precon(esp, A, kind)
    x0 = np.random.default_rng(2).standard_normal(A.n)
    got, log = run_device(esp, A, np.zeros(A.n), P, where)
    assert log["iters"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(log["resnorm"]) == 0 and not got.any()
    # cg! with b = 0 and x given has the residual -A*x: not this case; but maxiter = 0 leaves x untouched as well
    got, log = run_device(esp, A, np.zeros(A.n), P, where, x0=x0, maxiter=0)
    assert log["iters"] == 0 and not log["isconverged"] and same_bits(got, x0)
    close(P)


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_small_sizes(esp, orc, model, n):
    """n = 0, n = 1 and sizes beside the chunk of the summation shape"""
    A = esp.ExtendableSparseMatrix(n, n)
    if n > 0:
        d = np.arange(1, n + 1)
        A.append(esp.ESP_UPDATE, d, d, np.full(n, 4.0))
        if n > 1:
            A.append(esp.ESP_UPDATE, np.concatenate([d[1:], d[:-1]]), np.concatenate([d[:-1], d[1:]]), np.full(2 * n - 2, -1.0))
    A.flush()
    if n == 0:
        x, log = esp.cg(A, np.zeros(0), log=True)
        assert log["iters"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(x) == 0
        return
    arrays = host_arrays(A)
    b = np.random.default_rng(n).standard_normal(n)
    for kind in KIND_NAMES:
        check_against_model(model, orc, esp, A, arrays, kind, b, "host")


def test_value_change_then_update(esp, orc, model):
    """docs/src/iter.md:108-125: solve, change stored values in place, update!(preconditioner), solve again -- the second
    solve bitwise the model's on the NEW values"""
    A = esp.fdrand(20, 20, 1)
    n = A.n
    b = np.random.default_rng(7).random(n)
    P = esp.ILU0Preconditioner(A)
    arrays0 = host_arrays(A)
    x1, log1 = run_device(esp, A, b, P, "host")
    wx, wh, wit, wconv = model.cg(model.precon("ilu0", arrays0, orc), arrays0, b)
    assert same_bits(x1, wx) and same_bits(history_of(log1), wh)
    csc = A.sparse()                      # the reference's callers edit ext.cscmatrix.nzval in place
    cp, rv = csc.colptr, csc.rowval
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    csc.nzval[rv != cols] -= 1.0e-4       # every stored off-diagonal entry (symmetric)
    want_nz = np.array(csc.nzval, copy=True)
    P.update()
    x2, log2 = run_device(esp, A, b, P, "host")
    arrays1 = host_arrays(A)
    assert np.array_equal(bits(arrays1[2]), bits(want_nz)) and not np.array_equal(arrays1[2], arrays0[2])
    wx, wh, wit, wconv = model.cg(model.precon("ilu0", arrays1, orc), arrays1, b)
    assert log2["iters"] == wit and log2["isconverged"] and wconv
    assert same_bits(x2, wx) and same_bits(history_of(log2), wh)
    assert not same_bits(x1, x2)
    P.close()


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
def test_reference_acceptance(esp, orc, kind):
    """test_block.jl:14-36: A = fdrand(100, 100), b = A*ones, sol = cg(A, b, Pl = ...); sol ≈ ones"""
    A, arrays = oracle_matrix(esp, orc, "fdrand100x100")
    ones = np.ones(A.n)
    b = A.mul(ones)
    P = make_precon(esp, A, kind)
    sol, log = esp.cg(A, b, Pl=P, log=True)
    print("%s: %d iterations, |sol - 1|/sqrt(n) = %.3e" % (kind, log["iters"], np.linalg.norm(sol - ones) / math.sqrt(A.n)))
    assert log["isconverged"] and isapprox(sol, ones)
    assert np.array_equal(bits(esp.cg(A, b, Pl=P)), bits(sol))    # log=False returns x alone
    P.close()


def test_error_codes(esp):
    """include/esparse_hip.h, esp_cg: a preconditioner of another matrix, pending entries, a pattern change without update!,
    a rectangular matrix.  (The fourth row of the table, n or nnz >= 2^32 - 16, is the same check_handle every preconditioner
    call runs first; reaching it takes a matrix of 2^32 columns, 34 GB of column pointers alone: not exercised here.)"""
    A = esp.fdrand(8, 8, 8)
    B = esp.fdrand(8, 8, 8)
    n = A.n
    PA, PB = esp.ILU0Preconditioner(A), esp.JacobiPreconditioner(B)
    b = np.ones(n)
    with pytest.raises(ValueError):
        esp.cg(A, b, Pl=PB)
    lib = A._d.lib
    x = np.zeros(n)
    hist = np.zeros(n + 1)
    its, conv = ctypes.c_int64(), ctypes.c_int32()

    def call(h, p):
        return lib.esp_cg(h, p, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), 0, 1, n, 0.0, RELTOL,
                          hist.ctypes.data_as(ctypes.c_void_p), ctypes.byref(its), ctypes.byref(conv))

    assert call(A._d.h, PA._p) == 0 and conv.value == 1
    assert call(A._d.h, PB._p) == ESP_ERR_INVALID            # bound to another handle
    assert call(None, None) == ESP_ERR_INVALID
    assert lib.esp_cg(A._d.h, None, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), 0, 1, -1, 0.0, RELTOL,
                      None, None, None) == ESP_ERR_INVALID   # maxiter < 0
    assert lib.esp_cg(A._d.h, None, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), 0, 1, n, 0.0, RELTOL,
                      None, None, None) == 0                 # history, iterations, converged are optional
    A.append(esp.ESP_UPDATE, [1], [n], [0.5])                # pending entries: the C call does not flush
    assert call(A._d.h, PA._p) == ESP_ERR_STATE
    assert call(A._d.h, None) == ESP_ERR_STATE
    A.flush()                                                # a new position: the pattern changed
    assert call(A._d.h, PA._p) == ESP_ERR_STATE              # ... without update!
    assert call(A._d.h, None) == 0                           # (Identity has nothing to update)
    with pytest.raises(esp.EspError) as e:
        esp.cg(A, b, Pl=PA)
    assert e.value.code == ESP_ERR_STATE
    PA.update()
    assert call(A._d.h, PA._p) == 0
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    xr = np.zeros(5)
    assert lib.esp_cg(R._d.h, None, xr.ctypes.data_as(ctypes.c_void_p), xr.ctypes.data_as(ctypes.c_void_p), 0, 1, 3, 0.0, RELTOL,
                      None, None, None) == ESP_ERR_INVALID   # rectangular
    with pytest.raises(ValueError):
        esp.cg(A, np.ones(n + 1))
    with pytest.raises(ValueError):
        esp.cg(A, b, maxiter=-1)
    PA.close()
    PB.close()


def test_indefinite_and_breakdown(esp, orc, model):
    """no error on an indefinite matrix: a diagonal with one negative entry runs like any other; diag(1, -1) with b = (1, 1)
    breaks down in the first step (dot(u, c) = 0): Inf, then NaN, at the model's positions, until maxiter"""
    n = 600
    d = np.arange(1, n + 1)
    v = 1.0 + np.random.default_rng(3).random(n)
    v[17] = -v[17]
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, v)
    A.flush()
    b = np.random.default_rng(5).standard_normal(n)
    for kind in ("identity", "jacobi"):
        check_against_model(model, orc, esp, A, host_arrays(A), kind, b, "host", maxiter=6)
    D = esp.ExtendableSparseMatrix(2, 2)
    D.append(esp.ESP_UPDATE, [1, 2], [1, 2], [1.0, -1.0])
    D.flush()
    for where in ("host", "torch"):
        got, log = check_against_model(model, orc, esp, D, host_arrays(D), "identity", np.array([1.0, 1.0]), where, maxiter=4)
        h = history_of(log)
        assert log["iters"] == 4 and not log["isconverged"] and np.isinf(h[1]) and np.isnan(h[2:]).all() and np.isnan(got).all()


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_nonsymmetric_pattern(esp, orc, model, kind):
    """a non-symmetric pattern for 5 iterations: CG need not converge there, the arithmetic must still match"""
    A = nonsymmetric(esp)
    arrays = host_arrays(A)
    b = np.random.default_rng(9).standard_normal(A.n)
    check_against_model(model, orc, esp, A, arrays, kind, b, "torch", maxiter=5)


@pytest.mark.parametrize("kind", ["ilu0", "jacobi"])
def test_full_size_256(esp, orc, model, kind):
    """256^3 on device tensors: three iterations bitwise the model's, then a full solve to reltol = 1e-8 (maxiter = 10000
    only limits the test's time): converged, the last recurrence norm within tol.  Printed, not asserted: the iteration count
    and the true residual |b - A*x| (esp_mul) beside the recurrence's."""
    import torch
    nx = 256
    A = esp.fdrand(nx, nx, nx)
    arrays = host_arrays(A)
    n = A.n
    b = np.random.default_rng(8).standard_normal(n)
    P = make_precon(esp, A, kind)
    if kind == "ilu0":
        xd, idg = A.ilu0()      # (bit-identical to the oracle's ilu0: test_gpu_parity.py::test_jacobi_and_ilu0_setup)
        MP = Precon(KIND_ILU0, diag=np.ascontiguousarray(xd, np.float64), idiag=np.ascontiguousarray(idg, np.int64))
    else:                       # (... and test_jacobi_and_ilu0_setup for jacobi)
        MP = Precon(KIND_JACOBI, diag=np.ascontiguousarray(A.jacobi(), np.float64))
    tb = torch.from_numpy(b).cuda()
    got, log = esp.cg(A, tb, Pl=P, maxiter=3, reltol=0.0, log=True)
    wx, wh, wit, wconv = model.cg(MP, arrays, b, maxiter=3, reltol=0.0)
    assert log["iters"] == wit == 3 and not log["isconverged"]
    assert same_bits(history_of(log), wh)
    assert same_bits(got.cpu().numpy(), wx)
    x, log = esp.cg(A, tb, Pl=P, maxiter=10000, reltol=1e-8, log=True)
    h = history_of(log)
    tol = 1e-8 * h[0]
    true = torch.linalg.vector_norm(tb - A.mul(x)).item()
    print("256^3 %s: %d iterations, recurrence norm %.6e (tol %.6e), true residual %.6e, ratio %.4f"
          % (kind, log["iters"], h[-1], tol, true, true / h[-1]))
    assert log["isconverged"]
    assert h[-1] <= tol
    close(P)
