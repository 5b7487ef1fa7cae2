"""GPU: restarted GMRES on the device CSC (include/esparse_hip.h, esp_gmres; gmres of the package) against the model of
tests/gmres_model.c -- x, the whole residual history, the iteration, product and correction-pass counts and the convergence flag
bit for bit (a NaN equals a NaN at the same position): ldiv! and mul! are the reference's literal loops there, the dot products
the device's fixed summation shape restated on its own, the rotations and the back substitution written out."""
import ctypes
import math

import numpy as np
import pytest

import amg_modellib as am
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from edge_patterns import from_triplets, tridiagonal
from gmres_modellib import RELTOL, Model
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_STATE = -1, -6
KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
ORTHS = ["mgs", "cgs", "dgks"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("gmres_model"))


def host_arrays(A):
    """copies of the CSC arrays (the host copy behind A.sparse() is refreshed in place by later reads)"""
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def make_precon(esp, A, kind):
    return {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
            "iluam": esp.ILUAMPreconditioner}[kind](A)


def close(P):
    if P is not None:
        P.close()


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN (its payload is the hardware's business), at the same positions only"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


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


def run_device(esp, A, b, P, where, x0=None, **kw):
    """gmres (x0 None) or gmres! on host arrays or torch tensors -> (x as a NumPy array, log)"""
    if where == "host":
        x = None if x0 is None else x0.copy()
        got, log = esp.gmres(A, b, Pl=P, x=x, log=True, **kw)
        if x is not None:
            assert got is x
        return np.asarray(got), log
    import torch
    tx = None if x0 is None else torch.from_numpy(x0.copy()).cuda()
    got, log = esp.gmres(A, torch.from_numpy(np.ascontiguousarray(b)).cuda(), Pl=P, x=tx, log=True, **kw)
    if tx is not None:
        assert got.data_ptr() == tx.data_ptr()
    return got.cpu().numpy(), log


def compare(got, log, want, what=""):
    """x, the whole history, iters, mvps, reorth and isconverged bit for bit the model's"""
    print("%s: %d iterations (model %d), %d products (model %d), %d correction passes (model %d), converged %s, last norm %.3e"
          % (what, log["iters"], want.iters, log["mvps"], want.mvps, log["reorth"], want.reorth, log["isconverged"],
             history_of(log)[-1]))
    assert log["iters"] == want.iters and log["mvps"] == want.mvps and log["reorth"] == want.reorth
    assert log["isconverged"] == want.converged and len(log["resnorm"]) == want.iters
    assert same_bits(history_of(log), want.history)
    assert same_bits(got, want.x)


def check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=None, **kw):
    P = make_precon(esp, A, kind)
    try:
        got, log = run_device(esp, A, b, P, where, x0=x0, **kw)
        want = model.gmres(model.precon(kind, arrays, orc), arrays, b, x=x0, **kw)
        compare(got, log, want, "%s %s %s" % (kind, where, kw))
        return got, log
    finally:
        close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("name", ["fdrand20", "cd20"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_gmres_bitwise(esp, orc, model, kind, orth, name, where):
    """gmres(A, b; Pl, restart = 20) with b = A*ones to the default tolerance"""
    A, arrays, b = matrix(esp, orc, model, name)
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, where, restart=20, orth_meth=orth)
    assert log["isconverged"] and (orth == "dgks" or log["reorth"] == 0)
    if orth == "dgks" and name == "cd20" and kind in ("identity", "jacobi"):
        assert log["reorth"] > 0


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ["mgs", "dgks"])
@pytest.mark.parametrize("name", ["cd100x100", "nonsymmetric"])
def test_other_patterns(esp, orc, model, kind, orth, name):
    """a two-dimensional matrix, and row blocks above the staging capacity of the row kernels (the unstaged row branch)"""
    A, arrays, b = matrix(esp, orc, model, name)
    if name == "nonsymmetric":
        b = np.random.default_rng(9).standard_normal(A.n)
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", restart=20, orth_meth=orth)
    assert log["isconverged"]


@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("restart", [1, 2, 5, 64])
def test_restart_lengths(esp, orc, model, orth, restart):
    """restart 1 (every iteration a cycle), 2, 5 and the largest, 64 (eight groups of eight trees in the batched dots)"""
    A, arrays, b = matrix(esp, orc, model, "cd20")
    got, log = check_against_model(model, orc, esp, A, arrays, "jacobi", b, "torch", restart=restart, orth_meth=orth, maxiter=150)
    assert log["iters"] == 150 or log["isconverged"]


@pytest.mark.parametrize("kind", ["ilu0", "jacobi"])
@pytest.mark.parametrize("orth", ORTHS)
def test_two_level1_groups(esp, orc, model, kind, orth):
    """41^3 = 68 921 rows (odd: the scalar tail): 270 chunks, so TWO groups at level 1 and two values at level 2 -- the smallest
    such size; 45 iterations are two full cycles and a partial one"""
    A, arrays, b = matrix(esp, orc, model, "cd41")
    assert (A.n + 255) // 256 == 270
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "torch", restart=20, orth_meth=orth, maxiter=45, reltol=0.0)
    assert log["iters"] == 45 and log["mvps"] == 47


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
def test_truncation(esp, orc, model, kind, orth):
    """maxiter against restart = 5: the history is a prefix of the full run's, x the model's, the mid-cycle update included"""
    A, arrays, b = matrix(esp, orc, model, "cd20")
    restart = 5
    P = make_precon(esp, A, kind)
    MP = model.precon(kind, arrays, orc)
    full = None
    for limit in (2 * restart + 3, 0, 1, restart - 1, restart, restart + 1):
        got, log = run_device(esp, A, b, P, "torch", restart=restart, orth_meth=orth, maxiter=limit, reltol=0.0)
        want = model.gmres(MP, arrays, b, restart=restart, orth_meth=orth, maxiter=limit, reltol=0.0)
        compare(got, log, want, "%s %s maxiter=%d" % (kind, orth, limit))
        full = history_of(log) if full is None else full
        assert log["iters"] == limit and not log["isconverged"] and same_bits(history_of(log), full[:limit + 1])
        assert log["mvps"] == limit + (max(limit, 1) - 1) // restart
    close(P)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_inplace_from_a_random_start(esp, orc, model, kind, where):
    """gmres!(x, A, b; Pl): V1 = Pl \\ (b - A*x) first (one product more), x updated in place"""
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    rng = np.random.default_rng(21)
    b = rng.standard_normal(A.n)
    x0 = rng.standard_normal(A.n)
    for orth in ("mgs", "dgks"):
        got, log = check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=x0, restart=20, orth_meth=orth)
        assert log["mvps"] == log["iters"] + 1 + (log["iters"] - 1) // 20
    got, log = check_against_model(model, orc, esp, A, arrays, kind, b, where, x0=x0, maxiter=0)
    assert log["iters"] == 0 and log["mvps"] == 1 and not log["isconverged"] and same_bits(got, x0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 513])
def test_small_sizes(esp, orc, model, n):
    """sizes beside the chunk of the summation shape and the pair of chunks a workgroup of the MGS step takes; n = 1 is a lucky
    breakdown after one iteration: history [beta, 0], x exact; the default restart is min(20, n)"""
    A = tridiagonal(esp, n)
    arrays = host_arrays(A)
    b = np.random.default_rng(n).standard_normal(n) if n > 1 else np.array([2.0])   # (a power of two: V1 = 1 exactly)
    for kind in KIND_NAMES:
        for orth in ORTHS:
            got, log = check_against_model(model, orc, esp, A, arrays, kind, b, "host", orth_meth=orth)
            assert log["isconverged"]
            if n == 1:
                assert log["iters"] == 1 and log["resnorm"][0] == 0.0 and got[0] == b[0] / 4.0


def test_empty_matrix_and_zero_right_hand_side(esp, orc, model):
    """n = 0: history [0], nothing runs; b = 0 from x = 0: no iteration, x untouched, converged"""
    A = tridiagonal(esp, 0)
    for kind in KIND_NAMES:
        P = make_precon(esp, A, kind)
        for orth in ORTHS:
            x, log = esp.gmres(A, np.zeros(0), Pl=P, orth_meth=orth, log=True)
            assert log["iters"] == 0 and log["mvps"] == 0 and log["reorth"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(x) == 0
        close(P)
    A, _, _ = matrix(esp, orc, model, "cd20")
    for kind in KIND_NAMES:
        P = make_precon(esp, A, kind)
        for where in ("host", "torch"):
            got, log = run_device(esp, A, np.zeros(A.n), P, where)
            assert log["iters"] == 0 and log["mvps"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(log["resnorm"]) == 0
            assert not got.any()
        close(P)


@pytest.mark.parametrize("orth", ORTHS)
def test_restart_above_n_is_a_lucky_breakdown(esp, orc, model, orth):
    """restart = 20 > n = 3: the Krylov space is exhausted at iteration 3 at the latest; x solves the system"""
    A = tridiagonal(esp, 3)
    arrays = host_arrays(A)
    b = np.array([1.0, -2.0, 0.5])
    for where in ("host", "torch"):
        got, log = check_against_model(model, orc, esp, A, arrays, "identity", b, where, restart=20, orth_meth=orth, maxiter=10)
        assert log["iters"] <= 3 and log["isconverged"]
        assert np.allclose(model.mul(arrays, got), b, rtol=0, atol=1e-14)


def test_breakdown(esp, orc, model):
    """[0 0; 1 0] with every entry stored (a zero stored row) and b = e1: the first step gives V2 = e2 and no progress, the second
    A*e2 = 0 exactly -- nrm = 0 without convergence: 0/0 in the residual recurrence, a singular H in the update.  The NaNs sit at
    the model's positions and the loop ends at maxiter, no error"""
    D = esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(2, 2, np.array([1, 3, 5], np.int64), np.array([1, 2, 1, 2], np.int64),
                                                       np.array([0.0, 1.0, 0.0, 0.0])))
    arrays = host_arrays(D)
    assert len(arrays[2]) == 4
    for where in ("host", "torch"):
        for orth in ORTHS:
            got, log = check_against_model(model, orc, esp, D, arrays, "identity", np.array([1.0, 0.0]), where, restart=2, orth_meth=orth,
                                           maxiter=7)
            h = history_of(log)
            assert log["iters"] == 7 and not log["isconverged"] and list(h[:2]) == [1.0, 1.0] and np.isnan(h[2:]).all()
            assert np.isnan(got).any()


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
def test_two_runs_identical(esp, orc, model, kind, orth):
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    b = np.random.default_rng(4).standard_normal(A.n)
    P = make_precon(esp, A, kind)
    x1, l1 = run_device(esp, A, b, P, "torch", restart=10, orth_meth=orth, maxiter=25)
    x2, l2 = run_device(esp, A, b, P, "torch", restart=10, orth_meth=orth, maxiter=25)
    assert same_bits(x1, x2) and same_bits(history_of(l1), history_of(l2)) and l1["iters"] == l2["iters"] > 0
    assert l1["reorth"] == l2["reorth"] and l1["mvps"] == l2["mvps"]
    close(P)


def interleaved(n):
    """two partitions, the first not increasing (1, 5, 9, .., 3, 7, 11, ..): the permuted path"""
    return [np.concatenate([np.arange(1, n, 4), np.arange(3, n, 4)]), np.arange(0, n, 2)]


@pytest.mark.parametrize("which", ["ranges", "interleaved"])
@pytest.mark.parametrize("orth", ORTHS)
def test_block_preconditioner(esp, orc, model, which, orth):
    """Pl = BlockPreconditioner with ILU0 inside, on a range partitioning (the identity path) and an interleaved one (the permuted
    path: gather, inner ldiv!, scatter, then dot_k), through model_gmres_cb with the block model's ldiv"""
    A, arrays, b = matrix(esp, orc, model, "fdrand20")
    n = A.n
    parts = [np.arange(0, 3000), np.arange(3000, n)] if which == "ranges" else interleaved(n)
    P = esp.BlockPreconditioner(A, [p + 1 for p in parts], esp.ILU0Preconditioner)
    assert P.path == (0 if which == "ranges" else 1)
    BM = BlockModel(model, orc, "ilu0", arrays, parts)
    want = model.gmres_cb(BM, n, b, restart=20, orth_meth=orth)
    for where in ("host", "torch"):
        got, log = run_device(esp, A, b, P, where, restart=20, orth_meth=orth)
        compare(got, log, want, "block %s %s %s" % (which, orth, where))
    assert log["isconverged"]
    P.close()


@pytest.fixture(scope="module")
def amg20(esp, orc, model, tmp_path_factory):
    """the model hierarchy of fdrand 20 x 20 x 20 with the defaults: computed once, shared, left unchanged"""
    _, arrays, _ = matrix(esp, orc, model, "fdrand20")
    return am.AMGModel(am.Model(tmp_path_factory.mktemp("amg_model")), arrays)


@pytest.mark.parametrize("orth", ORTHS)
def test_amg_preconditioner(esp, orc, model, amg20, orth):
    """Pl = AMGPreconditioner: the V-cycle's launches in front of dot_k, through model_gmres_cb with the AMG model's ldiv"""
    A, arrays, _ = matrix(esp, orc, model, "fdrand20")
    b = np.random.default_rng(12).standard_normal(A.n)   # (A*ones is solved by one V-cycle: the prolongations keep constants)
    P = esp.AMGPreconditioner(A)
    want = model.gmres_cb(amg20, A.n, b, restart=20, orth_meth=orth)
    assert want.iters > 3
    for where in ("host", "torch"):
        got, log = run_device(esp, A, b, P, where, restart=20, orth_meth=orth)
        compare(got, log, want, "amg %s %s" % (orth, where))
    assert log["isconverged"]
    P.close()


def test_value_change_then_update(esp, orc, model):
    """docs/src/iter.md:97-102 with gmres: solve with ILU0, change stored values in place, update!(preconditioner), solve again --
    both solves converged and bitwise the model's on the old and the new values, the solutions differ"""
    A = convdiff(esp, 20, 20, 1, 2.0)
    n = A.n
    b = np.random.default_rng(7).random(n)
    P = esp.ILU0Preconditioner(A)
    arrays0 = host_arrays(A)
    x1, log1 = run_device(esp, A, b, P, "host")
    compare(x1, log1, model.gmres(model.precon("ilu0", arrays0, orc), arrays0, b), "before")
    assert log1["isconverged"]
    csc = A.sparse()                      # the reference's callers edit ext.cscmatrix.nzval in place
    cp, rv = csc.colptr, csc.rowval
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    csc.nzval[rv != cols] -= 1.0e-2       # every stored off-diagonal entry
    want_nz = np.array(csc.nzval, copy=True)
    P.update()
    x2, log2 = run_device(esp, A, b, P, "host")
    arrays1 = host_arrays(A)
    assert np.array_equal(bits(arrays1[2]), bits(want_nz)) and not np.array_equal(arrays1[2], arrays0[2])
    compare(x2, log2, model.gmres(model.precon("ilu0", arrays1, orc), arrays1, b), "after")
    assert log2["isconverged"] and not same_bits(x1, x2)
    P.close()


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_solves_convection_diffusion(esp, orc, model, kind):
    """the reason for the solver: convection-diffusion 20^3, Pe = 2, b = A*ones, reltol = 1e-10 -- converged, sol ≈ ones, the
    residual never grows; log=False returns x alone"""
    A, arrays, _ = matrix(esp, orc, model, "cd20")
    ones = np.ones(A.n)
    b = A.mul(ones)
    P = make_precon(esp, A, kind)
    for orth in ("mgs", "dgks"):
        sol, log = esp.gmres(A, b, Pl=P, reltol=1e-10, orth_meth=orth, log=True)
        print("%s %s: %d iterations, |b - A*x|/|b| = %.3e" % (kind, orth, log["iters"], np.linalg.norm(b - A.mul(sol)) / np.linalg.norm(b)))
        assert log["isconverged"] and np.linalg.norm(sol - ones) <= math.sqrt(np.finfo(np.float64).eps) * np.linalg.norm(ones)
        assert np.all(np.diff(history_of(log)) <= 0.0)
        assert np.array_equal(bits(esp.gmres(A, b, Pl=P, reltol=1e-10, orth_meth=orth)), bits(sol))
    close(P)


def test_error_codes(esp):
    """include/esparse_hip.h, esp_gmres: esp_bicgstabl's table (a preconditioner of another matrix, pending entries, a pattern
    change without update!, a rectangular matrix), restart outside 1..64, an unknown orth_meth, maxiter < 0, every out pointer
    NULL, and the wrapper's type and shape errors"""
    A = esp.fdrand(8, 8, 8)
    B = esp.fdrand(8, 8, 8)
    n = A.n
    PA, PB = esp.ILU0Preconditioner(A), esp.JacobiPreconditioner(B)
    b = np.ones(n)
    with pytest.raises(ValueError):
        esp.gmres(A, b, Pl=PB)
    lib = A._d.lib
    x = np.zeros(n)
    hist = np.zeros(n + 1)
    its, mvs, re, conv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    vb, vx = b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)

    def call(h, p, restart=20, orth=0, limit=n):
        x[:] = 0.0
        return lib.esp_gmres(h, p, vb, vx, 0, 1, restart, orth, limit, 0.0, RELTOL, hist.ctypes.data_as(ctypes.c_void_p),
                             ctypes.byref(its), ctypes.byref(mvs), ctypes.byref(re), ctypes.byref(conv))

    assert call(A._d.h, PA._p) == 0 and conv.value == 1 and mvs.value == its.value + (its.value - 1) // 20 and re.value == 0
    assert call(A._d.h, PB._p) == ESP_ERR_INVALID            # bound to another handle
    assert call(None, None) == ESP_ERR_INVALID
    assert call(A._d.h, None, limit=-1) == ESP_ERR_INVALID   # maxiter < 0
    for restart in (0, 65, -1):
        assert call(A._d.h, None, restart=restart) == ESP_ERR_INVALID    # 1 <= restart <= 64
        with pytest.raises(esp.EspError) as e:
            esp.gmres(A, b, restart=restart)
        assert e.value.code == ESP_ERR_INVALID
    for orth in (3, -1):
        assert call(A._d.h, None, orth=orth) == ESP_ERR_INVALID
    with pytest.raises(ValueError):
        esp.gmres(A, b, orth_meth="householder")
    for restart in (1, 64):
        for orth in (0, 1, 2):
            assert call(A._d.h, PA._p, restart=restart, orth=orth) == 0 and conv.value == 1
    assert lib.esp_gmres(A._d.h, None, vb, vx, 0, 1, 20, 2, n, 0.0, RELTOL, None, None, None, None, None) == 0   # all optional
    A.append(esp.ESP_UPDATE, [1], [n], [0.5])                # pending entries: the C call does not flush
    assert call(A._d.h, PA._p) == ESP_ERR_STATE
    assert call(A._d.h, None) == ESP_ERR_STATE
    A.flush()                                                # a new position: the pattern changed
    assert call(A._d.h, PA._p) == ESP_ERR_STATE              # ... without update!
    assert call(A._d.h, None) == 0                           # (Identity has nothing to update)
    with pytest.raises(esp.EspError) as e:
        esp.gmres(A, b, Pl=PA)
    assert e.value.code == ESP_ERR_STATE
    PA.update()
    assert call(A._d.h, PA._p) == 0
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    xr = np.zeros(5)
    vr = xr.ctypes.data_as(ctypes.c_void_p)
    assert lib.esp_gmres(R._d.h, None, vr, vr, 0, 1, 3, 0, 3, 0.0, RELTOL, None, None, None, None, None) == ESP_ERR_INVALID   # rectangular
    with pytest.raises(ValueError):
        esp.gmres(A, np.ones(n + 1))
    with pytest.raises(ValueError):
        esp.gmres(A, b, maxiter=-1)
    with pytest.raises(TypeError):
        esp.gmres(np.eye(3), np.ones(3))
    PA.close()
    PB.close()
