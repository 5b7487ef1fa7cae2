"""GPU: BiCGStab(l) on the device CSC (include/esparse_hip.h, esp_bicgstabl; bicgstabl of the package) against the model of
tests/bicgstabl_model.c -- x, the whole residual history, the iteration and product counts and the convergence flag bit for bit:
ldiv! and mul! are the reference's literal loops there, the dot products the device's fixed summation shape restated on its own,
the minimal-residual system an LU without pivoting written out."""
import ctypes
import math

import numpy as np
import pytest

from bicgstabl_modellib import RELTOL, Model, convdiff_triplets
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_STATE = -1, -6
KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("bicgstabl_model"))


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


def from_triplets(esp, n, I, J, V):
    A = esp.ExtendableSparseMatrix(n, n)
    if len(I):
        A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def convdiff(esp, nx, ny, nz, pe):
    """the upwind convection-diffusion matrix, built through append + flush"""
    return from_triplets(esp, nx * ny * nz, *convdiff_triplets(nx, ny, nz, pe))


def nonsymmetric(esp, n=3000, extra=20000, seed=5):
    """a non-symmetric matrix with a random extra pattern, every diagonal stored, built from appended triplets; its 256-row
    blocks exceed 2048 entries in places: the unstaged branch of the row kernels"""
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


def tridiagonal(esp, n):
    """the non-symmetric tridiagonal (4, -1.5 below, -0.5 above)"""
    d = np.arange(1, n + 1)
    I = np.concatenate([d, d[1:], d[:-1]])
    J = np.concatenate([d, d[:-1], d[1:]])
    V = np.concatenate([np.full(n, 4.0), np.full(max(n - 1, 0), -1.5), np.full(max(n - 1, 0), -0.5)])
    return from_triplets(esp, n, I, J, V)


MATRICES = {}   # name -> (A, arrays, b = A*ones): built once, never changed


def matrix(esp, orc, model, name):
    if name not in MATRICES:
        if name == "fdrand20":
            A = esp.fdrand(20, 20, 20)
            O = orc.fdrand(20, 20, 20, style=orc.KIND_UPDATE)
            arrays = host_arrays(A)
            for got, want in zip(arrays, O.sparse().arrays()):
                assert np.array_equal(bits(got) if got.dtype == np.float64 else got, bits(want) if want.dtype == np.float64 else want)
        else:
            A = {"cd20": lambda: convdiff(esp, 20, 20, 20, 2.0), "cd100x100": lambda: convdiff(esp, 100, 100, 1, 1.0),
                 "cd41": lambda: convdiff(esp, 41, 41, 41, 2.0), "nonsymmetric": lambda: nonsymmetric(esp)}[name]()
            arrays = host_arrays(A)
        MATRICES[name] = (A, arrays, model.mul(arrays, np.ones(A.n)))
    return MATRICES[name]


def run_device(esp, A, b, P, where, x0=None, r_shadow=None, **kw):
    """bicgstabl (x0 None) or bicgstabl! on host arrays or torch tensors -> (x as a NumPy array, log)"""
    if where == "host":
        x = None if x0 is None else x0.copy()
        got, log = esp.bicgstabl(A, b, Pl=P, x=x, r_shadow=r_shadow, log=True, **kw)
        if x is not None:
            assert got is x
        return np.asarray(got), log
    import torch
    tx = None if x0 is None else torch.from_numpy(x0.copy()).cuda()
    ts = None if r_shadow is None else torch.from_numpy(np.ascontiguousarray(r_shadow)).cuda()
    got, log = esp.bicgstabl(A, torch.from_numpy(np.ascontiguousarray(b)).cuda(), Pl=P, x=tx, r_shadow=ts, log=True, **kw)
    if tx is not None:
        assert got.data_ptr() == tx.data_ptr()
    return got.cpu().numpy(), log


def check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=None, **kw):
    """x, the whole history, iters, mvps and isconverged bit for bit the model's"""
    P = make_precon(esp, A, kind)
    try:
        got, log = run_device(esp, A, b, P, where, x0=x0, **kw)
        wx, wh, wit, wmv, wconv = model.bicgstabl(model.precon(kind, arrays, orc), arrays, b, x=x0, **kw)
        print("%s %s l=%s: %d outer iterations (model %d), %d products (model %d), converged %s, last norm %.3e"
              % (kind, where, kw.get("l", 2), log["iters"], wit, log["mvps"], wmv, log["isconverged"], history_of(log)[-1]))
        assert log["iters"] == wit and log["mvps"] == wmv and log["isconverged"] == wconv and len(log["resnorm"]) == wit
        assert same_bits(history_of(log), wh)
        assert same_bits(got, wx)
        return got, log
    finally:
        close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("l", [1, 2, 4])
@pytest.mark.parametrize("name", ["cd20", "cd100x100", "fdrand20"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_bicgstabl_bitwise(esp, orc, model, kind, l, name, where):
    """bicgstabl(A, b, l; Pl) with b = A*ones to the default tolerance"""
    A, arrays, b = matrix(esp, orc, model, name)
    check_against_model(model, orc, esp, A, arrays, kind, b, where, l=l)


@pytest.mark.parametrize("kind", ["ilu0", "jacobi"])
def test_two_level1_groups(esp, orc, model, kind):
    """41^3 = 68 921 rows: 270 chunks, so TWO groups at level 1 and two values at level 2 -- the smallest such size"""
    A, arrays, b = matrix(esp, orc, model, "cd41")
    assert (A.n + 255) // 256 == 270
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", l=2, max_mv_products=12)
    assert log["iters"] == 3 and log["mvps"] == 12


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("l", [1, 2])
def test_nonsymmetric_pattern(esp, orc, model, kind, l):
    """row blocks above the staging capacity of the row kernels"""
    A, arrays, _ = matrix(esp, orc, model, "nonsymmetric")
    b = np.random.default_rng(9).standard_normal(A.n)
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", l=l)
    assert log["isconverged"]


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("l", [1, 2, 4])
def test_truncation(esp, orc, model, kind, l):
    """max_mv_products is tested before an outer iteration, not inside it (reltol = 0: nothing but the limit ends the loop --
    at the default tolerance ILUAM with l = 4 converges within 6l products)"""
    A, arrays, b = matrix(esp, orc, model, "cd20")
    for limit, outer in ((1, 1), (2 * l, 1), (2 * l + 1, 2), (6 * l, 3)):
        got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", l=l, max_mv_products=limit, reltol=0.0)
        assert log["iters"] == outer and log["mvps"] == 2 * l * outer and not log["isconverged"]
    x0 = np.random.default_rng(1).standard_normal(A.n)   # x given: mv is 1 already, no iteration
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", x0=x0, l=l, max_mv_products=1)
    assert log["iters"] == 0 and log["mvps"] == 1 and not log["isconverged"] and same_bits(got, x0)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_inplace_from_a_random_start(esp, orc, model, kind, where):
    """bicgstabl!(x, A, b, l; Pl): rs[0] = Pl \\ (b - A*x) first, x updated in place"""
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    rng = np.random.default_rng(21)
    b = rng.standard_normal(A.n)
    check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=rng.standard_normal(A.n), l=2)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_r_shadow_given(esp, orc, model, kind, where):
    A, arrays, b = matrix(esp, orc, model, "cd20")
    rsh = np.random.default_rng(3).random(A.n)
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, where, l=2, r_shadow=rsh, max_mv_products=40)
    P = make_precon(esp, A, kind)
    other, olog = run_device(esp, A, b, P, where, l=2, max_mv_products=40)
    close(P)
    assert not same_bits(history_of(log), history_of(olog))


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_two_runs_identical(esp, orc, model, kind):
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    b = np.random.default_rng(4).standard_normal(A.n)
    P = make_precon(esp, A, kind)
    x1, l1 = run_device(esp, A, b, P, "torch", l=4, max_mv_products=48)
    x2, l2 = run_device(esp, A, b, P, "torch", l=4, max_mv_products=48)
    assert same_bits(x1, x2) and same_bits(history_of(l1), history_of(l2)) and l1["iters"] == l2["iters"] > 0
    close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_zero_right_hand_side(esp, orc, model, kind, where):
    """b = 0: residual 0 <= tol 0 -- no iteration, x untouched, converged"""
    A, _, _ = matrix(esp, orc, model, "cd20")
    P = make_precon(esp, A, kind)
    got, log = run_device(esp, A, np.zeros(A.n), P, where)
    assert log["iters"] == 0 and log["mvps"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(log["resnorm"]) == 0
    assert not got.any()
    x0 = np.random.default_rng(2).standard_normal(A.n)
    got, log = run_device(esp, A, np.zeros(A.n), P, where, x0=x0, max_mv_products=0)
    assert log["iters"] == 0 and not log["isconverged"] and same_bits(got, x0)
    close(P)


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_small_sizes(esp, orc, model, n):
    """n = 0; n = 1, where the first BiCG step solves exactly and the minimal-residual system is 0/0: NaN on both sides; sizes
    beside the chunk of the summation shape"""
    A = tridiagonal(esp, n)
    if n == 0:
        for kind in KIND_NAMES:
            P = make_precon(esp, A, kind)
            for l in (1, 2, 4):
                x, log = esp.bicgstabl(A, np.zeros(0), l=l, Pl=P, log=True)
                assert log["iters"] == 0 and log["mvps"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(x) == 0
            close(P)
        return
    arrays = host_arrays(A)
    b = np.random.default_rng(n).standard_normal(n)
    for kind in KIND_NAMES:
        for l in (1, 2, 4):
            got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "host", l=l)
            if n == 1:
                assert np.isnan(got).all() and np.isnan(log["resnorm"]).all() and not log["isconverged"]


def test_breakdown(esp, orc, model):
    """diag(1, -1) with b = (1, 1): dot(rt, A*rt) = 0 in the first step: Inf and NaN at the model's positions until
    max_mv_products, no error"""
    D = from_triplets(esp, 2, np.array([1, 2]), np.array([1, 2]), np.array([1.0, -1.0]))
    for where in ("host", "torch"):
        for l in (1, 2, 4):
            got, log = check_against_model(model, orc, esp, D, host_arrays(D), "identity", np.array([1.0, 1.0]), where, l=l,
                                           max_mv_products=8)
            h = history_of(log)
            assert log["mvps"] == 8 and log["iters"] == 8 // (2 * l) and not log["isconverged"]
            assert not np.isfinite(h[1:]).any() and np.isnan(got).all()


def test_value_change_then_update(esp, orc, model):
    """docs/src/iter.md:97-102: bicgstabl(A, b, 1; Pl = ILU0), then change stored values in place, update!(preconditioner), solve
    again -- both solves converged and bitwise the model's on the old and the new values, the solutions differ"""
    A = convdiff(esp, 20, 20, 1, 2.0)
    n = A.n
    b = np.random.default_rng(7).random(n)
    P = esp.ILU0Preconditioner(A)
    arrays0 = host_arrays(A)
    x1, log1 = run_device(esp, A, b, P, "host", l=1)
    wx, wh, wit, wmv, wconv = model.bicgstabl(model.precon("ilu0", arrays0, orc), arrays0, b, l=1)
    assert log1["isconverged"] and wconv and log1["iters"] == wit and log1["mvps"] == wmv
    assert same_bits(x1, wx) and same_bits(history_of(log1), wh)
    csc = A.sparse()                      # the reference's callers edit ext.cscmatrix.nzval in place
    cp, rv = csc.colptr, csc.rowval
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    csc.nzval[rv != cols] -= 1.0e-2       # every stored off-diagonal entry
    want_nz = np.array(csc.nzval, copy=True)
    P.update()
    x2, log2 = run_device(esp, A, b, P, "host", l=1)
    arrays1 = host_arrays(A)
    assert np.array_equal(bits(arrays1[2]), bits(want_nz)) and not np.array_equal(arrays1[2], arrays0[2])
    wx, wh, wit, wmv, wconv = model.bicgstabl(model.precon("ilu0", arrays1, orc), arrays1, b, l=1)
    assert log2["isconverged"] and wconv and log2["iters"] == wit and log2["mvps"] == wmv
    assert same_bits(x2, wx) and same_bits(history_of(log2), wh)
    assert not same_bits(x1, x2)
    P.close()


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_solves_what_cg_cannot(esp, orc, model, kind):
    """the reason for the solver: convection-diffusion 20^3, Pe = 2, b = A*ones, reltol = 1e-10 -- converged, sol ≈ ones.  The
    true residual and, as information only, cg on the same system after 200 iterations are printed."""
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    ones = np.ones(A.n)
    b = A.mul(ones)
    nb = np.linalg.norm(b)
    P = make_precon(esp, A, kind)
    for l in (1, 2, 4):
        sol, log = esp.bicgstabl(A, b, l=l, Pl=P, reltol=1e-10, log=True)
        print("%s l=%d: %d products, |b - A*x|/|b| = %.3e, |sol - 1|/sqrt(n) = %.3e"
              % (kind, l, log["mvps"], np.linalg.norm(b - A.mul(sol)) / nb, np.linalg.norm(sol - ones) / math.sqrt(A.n)))
        assert log["isconverged"] and isapprox(sol, ones)
        assert np.array_equal(bits(esp.bicgstabl(A, b, l=l, Pl=P, reltol=1e-10)), bits(sol))    # log=False returns x alone
    xc, clog = esp.cg(A, b, Pl=P, maxiter=200, log=True)
    print("%s cg, 200 iterations at most: %d run, converged %s, |b - A*x|/|b| = %.3e"
          % (kind, clog["iters"], clog["isconverged"], np.linalg.norm(b - A.mul(xc)) / nb))
    close(P)


def test_error_codes(esp):
    """include/esparse_hip.h, esp_bicgstabl: esp_cg's table (a preconditioner of another matrix, pending entries, a pattern change
    without update!, a rectangular matrix; n or nnz >= 2^32 - 16 is the same check_handle and not exercised, as there), an
    unsupported l, and the wrapper's type and shape errors"""
    A = esp.fdrand(8, 8, 8)
    B = esp.fdrand(8, 8, 8)
    n = A.n
    PA, PB = esp.ILU0Preconditioner(A), esp.JacobiPreconditioner(B)
    b = np.ones(n)
    with pytest.raises(ValueError):
        esp.bicgstabl(A, b, Pl=PB)
    lib = A._d.lib
    x = np.zeros(n)
    hist = np.zeros(n + 1)
    its, mvs, conv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    vb, vx = b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)

    def call(h, p, l=2, limit=n):
        return lib.esp_bicgstabl(h, p, l, vb, vx, None, 0, 1, limit, 0.0, RELTOL, hist.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.byref(its), ctypes.byref(mvs), ctypes.byref(conv))

    assert call(A._d.h, PA._p) == 0 and conv.value == 1 and mvs.value == 4 * its.value
    assert call(A._d.h, PB._p) == ESP_ERR_INVALID            # bound to another handle
    assert call(None, None) == ESP_ERR_INVALID
    assert call(A._d.h, None, limit=-1) == ESP_ERR_INVALID   # max_mv_products < 0
    for l in (0, 5, -1):
        assert call(A._d.h, None, l=l) == ESP_ERR_INVALID    # 1 <= l <= 4
        with pytest.raises(esp.EspError) as e:
            esp.bicgstabl(A, b, l=l)
        assert e.value.code == ESP_ERR_INVALID
    for l in (1, 2, 3, 4):
        assert call(A._d.h, PA._p, l=l) == 0 and conv.value == 1
    assert lib.esp_bicgstabl(A._d.h, None, 2, vb, vx, None, 0, 1, n, 0.0, RELTOL, None, None, None, None) == 0   # all optional
    A.append(esp.ESP_UPDATE, [1], [n], [0.5])                # pending entries: the C call does not flush
    assert call(A._d.h, PA._p) == ESP_ERR_STATE
    assert call(A._d.h, None) == ESP_ERR_STATE
    A.flush()                                                # a new position: the pattern changed
    assert call(A._d.h, PA._p) == ESP_ERR_STATE              # ... without update!
    assert call(A._d.h, None) == 0                           # (Identity has nothing to update)
    with pytest.raises(esp.EspError) as e:
        esp.bicgstabl(A, b, Pl=PA)
    assert e.value.code == ESP_ERR_STATE
    PA.update()
    assert call(A._d.h, PA._p) == 0
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    xr = np.zeros(5)
    vr = xr.ctypes.data_as(ctypes.c_void_p)
    assert lib.esp_bicgstabl(R._d.h, None, 2, vr, vr, None, 0, 1, 3, 0.0, RELTOL, None, None, None, None) == ESP_ERR_INVALID   # rectangular
    with pytest.raises(ValueError):
        esp.bicgstabl(A, np.ones(n + 1))
    with pytest.raises(ValueError):
        esp.bicgstabl(A, b, max_mv_products=-1)
    with pytest.raises(ValueError):
        esp.bicgstabl(A, b, r_shadow=np.ones(n + 1))
    import torch
    with pytest.raises(ValueError):
        esp.bicgstabl(A, torch.ones(n, dtype=torch.float64).cuda(), r_shadow=torch.ones(n + 1, dtype=torch.float64).cuda())
    with pytest.raises(TypeError):
        esp.bicgstabl(np.eye(3), np.ones(3))
    PA.close()
    PB.close()
