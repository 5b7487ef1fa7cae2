"""CPU: the model of restarted GMRES (tests/gmres_model.c) the GPU tests compare esp_gmres with bit for bit.  It follows an
independent NumPy restatement of the statements, keeps the Arnoldi relation, reports at every restart the residual the solution
it formed there really has, replays the reference's own non-symmetric test (test/test_parilu0.jl:16-17), and honours restart,
maxiter and the three orthogonalisations as include/esparse_hip.h states them."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from bicgstabl_modellib import convdiff_triplets, csc_arrays
from gmres_modellib import RELTOL, Model

KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
ORTHS = ["mgs", "cgs", "dgks"]
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("gmres_model"))


@pytest.fixture(scope="module")
def cd20():
    """convection-diffusion 20^3, Pe = 2"""
    return csc_arrays(20 ** 3, *convdiff_triplets(20, 20, 20, 2.0))


@pytest.fixture(scope="module")
def cd8():
    """convection-diffusion 8 x 7 x 3, Pe = 2: the small matrix of the statement-level tests"""
    return csc_arrays(8 * 7 * 3, *convdiff_triplets(8, 7, 3, 2.0))


def scipy_of(arrays):
    cp, rv, nz = arrays
    n = len(cp) - 1
    return sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).tocsr()


def isapprox(x, y):
    """Julia's x ≈ y for vectors: norm(x - y) <= sqrt(eps) * max(norm(x), norm(y))"""
    return np.linalg.norm(x - y) <= math.sqrt(EPS) * max(np.linalg.norm(x), np.linalg.norm(y))


def numpy_gmres(S, ldiv, b, restart, maxiter, reltol, orth="mgs"):
    """restarted GMRES the textbook way, written without a look at the model: Arnoldi with np.dot, the least-squares problem by
    np.linalg.lstsq, the residual norm as the norm of the least-squares residual -> (x, history)"""
    n = len(b)
    x = np.zeros(n)
    r = ldiv(b)
    beta = np.linalg.norm(r)
    hist = [beta]
    tol = reltol * beta
    it = 0
    while it < maxiter and not hist[-1] <= tol:
        V = np.zeros((n, restart + 1))
        H = np.zeros((restart + 1, restart))
        V[:, 0] = r / beta
        m = 0
        while m < restart and it < maxiter and not hist[-1] <= tol:
            w = ldiv(S @ V[:, m])
            if orth == "mgs":
                for i in range(m + 1):
                    H[i, m] = np.dot(V[:, i], w)
                    w = w - H[i, m] * V[:, i]
            else:
                h = V[:, :m + 1].T @ w
                w = w - V[:, :m + 1] @ h
                if orth == "dgks":
                    proj, passes = np.linalg.norm(h), 0
                    while np.linalg.norm(w) < proj / math.sqrt(2.0) and passes < 3:
                        c = V[:, :m + 1].T @ w
                        proj = np.linalg.norm(c)
                        w = w - V[:, :m + 1] @ c
                        h = h + c
                        passes += 1
                H[:m + 1, m] = h
            H[m + 1, m] = np.linalg.norm(w)
            V[:, m + 1] = w / H[m + 1, m]
            m += 1
            it += 1
            e1 = np.zeros(m + 1)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H[:m + 1, :m], e1, rcond=None)
            hist.append(np.linalg.norm(e1 - H[:m + 1, :m] @ y))
        x = x + V[:, :m] @ y
        r = ldiv(b - S @ x)
        beta = np.linalg.norm(r)
    return x, np.array(hist)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
def test_model_follows_a_numpy_restatement(orc, model, cd8, kind, orth):
    """three cycles of restart 6 against np.dot / np.linalg.lstsq: the orders of summation differ and the residual comes from the
    least-squares problem there, from the nullvec recurrence here -- the histories agree to a relative 1e-8 (plus 1e-13 of the
    initial norm, the floor below which neither carries a digit), x to 1e-8"""
    arrays = cd8
    n = len(arrays[0]) - 1
    S = scipy_of(arrays)
    b = model.mul(arrays, np.ones(n))
    P = model.precon(kind, arrays, orc)
    r = model.gmres(P, arrays, b, restart=6, orth_meth=orth, maxiter=18, reltol=0.0)
    wx, wh = numpy_gmres(S, lambda v: model.ldiv(P, arrays, v), b, 6, 18, 0.0, orth)
    assert r.iters == 18 == len(wh) - 1 and r.mvps == 18 + 2
    assert np.all(np.abs(r.history - wh) <= 1e-8 * np.abs(wh) + 1e-13 * wh[0])
    assert np.linalg.norm(r.x - wx) <= 1e-8 * np.linalg.norm(wx)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
def test_arnoldi_relation_and_orthonormal_basis(orc, model, cd20, kind, orth):
    """(Pl \\ A) V_m = V_{m+1} H to 1e-10 before the rotations on the last full cycle of a run of 40; with DGKS V'V = I to 1e-10"""
    arrays = cd20
    n = len(arrays[0]) - 1
    S = scipy_of(arrays)
    b = model.mul(arrays, np.ones(n))
    P = model.precon(kind, arrays, orc)
    r = model.gmres(P, arrays, b, restart=20, orth_meth=orth, maxiter=40, reltol=0.0, probe=True)
    assert r.iters == 40 and r.m == 20 and r.cycles == 2 and r.H.shape == (21, 20) and r.V.shape == (n, 21)
    AV = np.stack([model.ldiv(P, arrays, S @ r.V[:, j]) for j in range(20)], axis=1)
    assert np.abs(AV - r.V @ r.H).max() <= 1e-10 * np.abs(r.H).max()
    if orth == "dgks":   # (MGS loses orthogonality with the condition of the Krylov basis, CGS with its square: no bound is set)
        assert np.abs(r.V.T @ r.V - np.eye(21)).max() <= 1e-10
    assert np.all(np.tril(r.H, -2) == 0.0)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("orth", ORTHS)
def test_implicit_residual_is_the_true_one_at_every_restart(orc, model, cd20, kind, orth):
    """history[it] against norm(Pl \\ (b - A x)) of the x formed at iteration it, for every cycle (the last, partial one included)"""
    arrays = cd20
    n = len(arrays[0]) - 1
    S = scipy_of(arrays)
    b = model.mul(arrays, np.ones(n))
    P = model.precon(kind, arrays, orc)
    r = model.gmres(P, arrays, b, restart=7, orth_meth=orth, maxiter=38, reltol=0.0, probe=True)
    assert r.cycles == 6 and list(r.restart_it) == [7, 14, 21, 28, 35, 38]
    for xc, it in zip(r.restart_x, r.restart_it):
        true = np.linalg.norm(model.ldiv(P, arrays, b - S @ xc))
        assert abs(true - r.history[it]) <= 1e-10 * r.history[0]
    assert np.array_equal(r.restart_x[-1], r.x)
    assert np.all(np.diff(r.history) <= 0.0)          # GMRES's residual never grows


@pytest.mark.parametrize("n", [10, 100, 1000])
def test_parilu0_shape_replayed(orc, model, n):
    """test/test_parilu0.jl:16-17: sol = gmres(A, b; Pl = ilu0) on a strictly diagonally dominant matrix, sol ≈ ones"""
    rng = np.random.default_rng(n)
    S = sp.random(n, n, density=min(0.5, 5.0 / n), random_state=rng, format="lil")
    S.setdiag(0.0)
    S = sp.csr_matrix(S)
    S = S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)
    S = sp.coo_matrix(S)
    arrays = csc_arrays(n, S.row.astype(np.int64) + 1, S.col.astype(np.int64) + 1, S.data)
    b = model.mul(arrays, np.ones(n))
    for kind in ("ilu0", "iluam"):
        for orth in ORTHS:
            r = model.gmres(model.precon(kind, arrays, orc), arrays, b, orth_meth=orth)
            assert r.converged and r.iters <= n and isapprox(r.x, np.ones(n)), (kind, orth)


@pytest.mark.parametrize("orth", ORTHS)
def test_convection_diffusion_to_1e_10(orc, model, cd20, orth):
    """convdiff(20,20,20,2.0) with Jacobi and reltol = 1e-10: converged, x ≈ ones; MGS and DGKS take the 162 iterations a NumPy
    restatement with BLAS sums took (a few more or less: the order of summation differs)"""
    arrays = cd20
    n = len(arrays[0]) - 1
    b = model.mul(arrays, np.ones(n))
    r = model.gmres(model.precon("jacobi", arrays, orc), arrays, b, orth_meth=orth, reltol=1e-10)
    print(orth, r.iters, r.mvps, r.reorth)
    assert r.converged and isapprox(r.x, np.ones(n)) and (orth == "cgs" or abs(r.iters - 162) <= 3)
    assert r.mvps == r.iters + (r.iters - 1) // 20 and r.history[-1] <= 1e-10 * r.history[0] < r.history[-2]
    assert (r.reorth > 0) == (orth == "dgks")


def test_dgks_corrects_and_never_hits_the_cap(orc, model, cd20):
    """on cd20 DGKS makes at least one correction pass and never three in one step (the cap): run iteration by iteration, the
    pass counter never rises by 3"""
    arrays = cd20
    n = len(arrays[0]) - 1
    b = model.mul(arrays, np.ones(n))
    P = model.precon("jacobi", arrays, orc)
    counts = [model.gmres(P, arrays, b, orth_meth="dgks", maxiter=k, reltol=0.0).reorth for k in range(0, 41)]
    steps = np.diff(counts)
    assert counts[0] == 0 and counts[-1] >= 1 and steps.min() >= 0 and steps.max() < 3
    assert model.gmres(P, arrays, b, orth_meth="mgs", maxiter=40, reltol=0.0).reorth == 0
    assert model.gmres(P, arrays, b, orth_meth="cgs", maxiter=40, reltol=0.0).reorth == 0


def test_one_unknown_is_a_lucky_breakdown(orc, model):
    """n = 1: one iteration, history [beta, 0], x exact"""
    one = (np.array([1, 2], np.int64), np.array([1], np.int64), np.array([4.0]))
    for kind in ("identity", "jacobi", "ilu0"):
        for orth in ORTHS:
            r = model.gmres(model.precon(kind, one, orc), one, np.array([2.0]), orth_meth=orth)
            beta = 2.0 if kind == "identity" else 0.5
            assert r.iters == 1 and r.converged and list(r.history) == [beta, 0.0] and list(r.x) == [0.5] and r.mvps == 1


def test_zero_right_hand_side_and_empty_matrix(orc, model, cd8):
    arrays = cd8
    n = len(arrays[0]) - 1
    for kind in KIND_NAMES:
        r = model.gmres(model.precon(kind, arrays, orc), arrays, np.zeros(n))
        assert r.iters == 0 and r.mvps == 0 and r.converged and list(r.history) == [0.0] and not r.x.any()
    empty = (np.ones(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    r = model.gmres(model.precon("identity", empty, orc), empty, np.zeros(0))
    assert r.iters == 0 and r.converged and list(r.history) == [0.0] and len(r.x) == 0


@pytest.mark.parametrize("orth", ORTHS)
def test_restart_larger_than_n(orc, model, orth):
    """restart = 20 > n = 3: the Krylov space is exhausted at iteration 3 -- a lucky breakdown, x exact to rounding"""
    d = np.arange(1, 4)
    arrays = csc_arrays(3, np.concatenate([d, d[1:], d[:-1]]), np.concatenate([d, d[:-1], d[1:]]),
                        np.array([4.0, 4.0, 4.0, -1.5, -1.5, -0.5, -0.5]))
    S = scipy_of(arrays)
    b = np.array([1.0, -2.0, 0.5])
    r = model.gmres(model.precon("identity", arrays, orc), arrays, b, restart=20, orth_meth=orth, maxiter=10)
    assert r.iters == 3 and r.converged and r.mvps == 3
    assert np.allclose(S @ r.x, b, rtol=0, atol=1e-14)


@pytest.mark.parametrize("orth", ORTHS)
def test_truncation_rules(orc, model, cd20, orth):
    """maxiter is tested before every iteration; the history is a prefix of the full run's; x is formed when maxiter ends a cycle
    part-way, and then belongs to the residual reported; a new cycle is not begun (no product) when maxiter ends the run at a
    restart"""
    arrays = cd20
    n = len(arrays[0]) - 1
    S = scipy_of(arrays)
    b = model.mul(arrays, np.ones(n))
    P = model.precon("ilu0", arrays, orc)
    restart = 5
    full = model.gmres(P, arrays, b, restart=restart, orth_meth=orth, maxiter=2 * restart + 3, reltol=0.0)
    for limit in (0, 1, restart - 1, restart, restart + 1, 2 * restart + 3):
        r = model.gmres(P, arrays, b, restart=restart, orth_meth=orth, maxiter=limit, reltol=0.0)
        assert r.iters == limit and not r.converged and np.array_equal(r.history, full.history[:limit + 1])
        assert r.mvps == limit + (max(limit, 1) - 1) // restart
        true = np.linalg.norm(model.ldiv(P, arrays, b - S @ r.x))
        assert abs(true - r.history[-1]) <= 1e-10 * r.history[0]
    x0 = np.random.default_rng(1).standard_normal(n)      # x given: the initial residual costs a product
    r = model.gmres(P, arrays, b, x=x0, restart=restart, orth_meth=orth, maxiter=0)
    assert r.iters == 0 and r.mvps == 1 and not r.converged and np.array_equal(r.x, x0)
    r = model.gmres(P, arrays, b, x=x0, restart=restart, orth_meth=orth, maxiter=restart + 1, reltol=0.0)
    assert r.iters == restart + 1 and r.mvps == restart + 3


def test_refused_arguments(orc, model, cd8):
    arrays = cd8
    n = len(arrays[0]) - 1
    P = model.precon("identity", arrays, orc)
    for kw in ({"restart": 0}, {"restart": 65}, {"maxiter": -1}):
        with pytest.raises(AssertionError):
            model.gmres(P, arrays, np.ones(n), **kw)


def test_callbacks_run_the_same_loop(orc, model, cd8):
    """model_gmres_cb with Python callbacks around the model's own mul and ldiv is model_gmres bit for bit"""
    arrays = cd8
    n = len(arrays[0]) - 1
    b = np.random.default_rng(3).standard_normal(n)
    P = model.precon("ilu0", arrays, orc)

    class M:
        mul = staticmethod(lambda v: model.mul(arrays, v))
        ldiv = staticmethod(lambda v: model.ldiv(P, arrays, v))

    for orth in ORTHS:
        a = model.gmres(P, arrays, b, restart=4, orth_meth=orth, maxiter=11, reltol=0.0)
        c = model.gmres_cb(M, n, b, restart=4, orth_meth=orth, maxiter=11, reltol=0.0)
        assert np.array_equal(a.x, c.x) and np.array_equal(a.history, c.history)
        assert (a.iters, a.mvps, a.reorth, a.converged) == (c.iters, c.mvps, c.reorth, c.converged)


def test_least_squares_by_rotations(model):
    """the Givens rotations and the back substitution against np.linalg.lstsq on random Hessenberg matrices, and a literal 1 x 1"""
    rng = np.random.default_rng(8)
    for m in (1, 2, 5, 20, 64):
        H = np.triu(rng.standard_normal((m + 1, m)), -1)
        y = model.lsq(H, 3.0)
        e1 = np.zeros(m + 1)
        e1[0] = 3.0
        want, *_ = np.linalg.lstsq(H, e1, rcond=None)
        assert np.abs(y - want).max() <= 1e3 * EPS * np.linalg.cond(H) * np.abs(want).max()   # (both are backward stable)
    H = np.array([[3.0], [4.0]])
    c, s = 3.0 / 5.0, 4.0 / 5.0
    assert model.lsq(H, 2.0)[0] == (c * 2.0 + s * 0.0) / (c * 3.0 + s * 4.0)
    assert RELTOL == math.sqrt(EPS)
