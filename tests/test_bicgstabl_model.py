"""CPU: the model of BiCGStab(l) (tests/bicgstabl_model.c) the GPU tests compare esp_bicgstabl with bit for bit.  On an upwind
convection-diffusion matrix -- non-symmetric: conjugate gradients have no business there -- it converges for every l and
preconditioner to the reference's acceptance (`sol ≈ ones`), follows an independent NumPy restatement of the statements, and
honours r_shadow and max_mv_products as include/esparse_hip.h states them."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from bicgstabl_modellib import Model, convdiff_triplets, csc_arrays

KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("bicgstabl_model"))


@pytest.fixture(scope="module")
def cd20():
    """convection-diffusion 20^3, Pe = 2: (arrays, b = A*ones as scipy forms it)"""
    n = 20 ** 3
    return csc_arrays(n, *convdiff_triplets(20, 20, 20, 2.0))


def isapprox(x, y):
    """Julia's x ≈ y for vectors: norm(x - y) <= sqrt(eps) * max(norm(x), norm(y))"""
    return np.linalg.norm(x - y) <= math.sqrt(EPS) * max(np.linalg.norm(x), np.linalg.norm(y))


def numpy_bicgstabl(S, ldiv, b, l, outer, r_shadow=None):
    """the statements of include/esparse_hip.h with np.dot, S @ v and np.linalg.solve: the history of `outer` outer iterations"""
    n = len(b)
    rs = np.zeros((l + 1, n))
    us = np.zeros((l + 1, n))
    x = np.zeros(n)
    rs[0] = ldiv(b)
    rt = rs[0].copy() if r_shadow is None else r_shadow
    omega = sigma = 1.0
    hist = [np.linalg.norm(rs[0])]
    for _ in range(outer):
        sigma = -omega * sigma
        for j in range(l):
            rho = np.dot(rt, rs[j])
            beta = rho / sigma
            us[:j + 1] = rs[:j + 1] - beta * us[:j + 1]
            us[j + 1] = ldiv(S @ us[j])
            sigma = np.dot(rt, us[j + 1])
            alpha = rho / sigma
            rs[:j + 1] -= alpha * us[1:j + 2]
            rs[j + 1] = ldiv(S @ rs[j])
            x += alpha * us[0]
        M = rs @ rs.T
        gamma = np.linalg.solve(M[1:, 1:], M[1:, 0])
        us[0] -= gamma @ us[1:]
        x += gamma @ rs[:-1]
        rs[0] -= gamma @ rs[1:]
        omega = gamma[-1]
        hist.append(np.linalg.norm(rs[0]))
    return np.array(hist)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("l", [1, 2, 4])
def test_model_converges_on_convection_diffusion(orc, model, cd20, kind, l):
    """docs/src/iter.md:97-102 with the roles filled: b = A*ones, sol = bicgstabl(A, b, l; Pl, reltol = 1e-10), sol ≈ ones"""
    arrays = cd20
    n = len(arrays[0]) - 1
    ones = np.ones(n)
    b = model.mul(arrays, ones)
    P = model.precon(kind, arrays, orc)
    x, hist, it, mv, conv = model.bicgstabl(P, arrays, b, l=l, reltol=1e-10)
    print("%s l=%d: %d outer iterations, %d products, |x - 1|/sqrt(n) = %.3e" % (kind, l, it, mv, np.linalg.norm(x - ones) / math.sqrt(n)))
    assert conv and mv == 2 * l * it and mv < n and len(hist) == it + 1
    assert hist[-1] <= 1e-10 * hist[0]
    assert isapprox(x, ones)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("l", [1, 2, 4])
def test_model_follows_a_numpy_restatement(orc, model, cd20, kind, l):
    """the first five outer iterations of the solve to reltol = 1e-10 against np.dot / np.linalg.solve: the orders of summation
    and the pivoting differ, the histories agree to a relative 1e-6.  A solve that converges sooner (ILUAM with l = 4 needs four
    outer iterations) is compared over the iterations it runs: one more would compare two norms of 1e-16 beside an initial 28,
    below eps times the initial norm, where neither carries a correct digit."""
    arrays = cd20
    cp, rv, nz = arrays
    n = len(cp) - 1
    S = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).tocsr()
    b = model.mul(arrays, np.ones(n))
    P = model.precon(kind, arrays, orc)
    x, hist, it, mv, conv = model.bicgstabl(P, arrays, b, l=l, max_mv_products=10 * l, reltol=1e-10)
    assert mv == 2 * l * it and (it == 5 or (conv and 0 < it < 5))
    want = numpy_bicgstabl(S, lambda v: model.ldiv(P, arrays, v), b, l, it)
    print(kind, l, np.abs(hist - want) / np.abs(want))
    assert np.all(np.abs(hist - want) <= 1e-6 * np.abs(want))


def test_gamma_solves_the_minimal_residual_system(model):
    """the LU without pivoting against np.linalg.solve on Gram matrices of random vectors (symmetric positive definite: no pivot
    is needed), and its literal values for l = 1 and l = 2"""
    rng = np.random.default_rng(6)
    for l in (1, 2, 3, 4):
        R = rng.standard_normal((l + 1, 50))
        M = R @ R.T
        g = model.gamma(M)
        assert np.allclose(g, np.linalg.solve(M[1:, 1:], M[1:, 0]), rtol=1e-10, atol=0)
    M = np.array([[3.0, 5.0], [5.0, 7.0]])
    assert model.gamma(M)[0] == 5.0 / 7.0
    M = np.array([[9.0, 1.0, 2.0], [1.0, 4.0, 3.0], [2.0, 3.0, 8.0]])
    l21 = 3.0 * (1.0 / 4.0)
    u22 = 8.0 - l21 * 3.0
    y2 = 2.0 - l21 * 1.0
    g2 = y2 / u22
    assert list(model.gamma(M)) == [(1.0 - 3.0 * g2) / 4.0, g2]


def test_r_shadow_changes_the_history_and_none_is_the_default(orc, model, cd20):
    arrays = cd20
    n = len(arrays[0]) - 1
    b = model.mul(arrays, np.ones(n))
    P = model.precon("jacobi", arrays, orc)
    x0, h0, it0, mv0, c0 = model.bicgstabl(P, arrays, b, l=2, max_mv_products=24)
    default = model.ldiv(P, arrays, b)                      # the initial preconditioned residual
    x1, h1, it1, mv1, c1 = model.bicgstabl(P, arrays, b, l=2, max_mv_products=24, r_shadow=default)
    assert np.array_equal(x0, x1) and np.array_equal(h0, h1) and (it0, mv0, c0) == (it1, mv1, c1)
    rsh = np.random.default_rng(3).random(n)
    x2, h2, it2, mv2, c2 = model.bicgstabl(P, arrays, b, l=2, max_mv_products=24, r_shadow=rsh)
    assert h2[0] == h0[0] and it2 == it0 and not np.array_equal(h2[1:], h0[1:]) and not np.array_equal(x2, x0)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_max_mv_products_is_checked_before_an_outer_iteration(orc, model, cd20, l):
    arrays = cd20
    n = len(arrays[0]) - 1
    b = model.mul(arrays, np.ones(n))
    P = model.precon("identity", arrays, orc)
    _, full, _, _, _ = model.bicgstabl(P, arrays, b, l=l, max_mv_products=6 * l)
    for limit, outer in ((0, 0), (1, 1), (2 * l, 1), (2 * l + 1, 2), (6 * l, 3)):
        x, hist, it, mv, conv = model.bicgstabl(P, arrays, b, l=l, max_mv_products=limit)
        assert it == outer and mv == 2 * l * outer and not conv and np.array_equal(hist, full[:outer + 1])
    x0 = np.random.default_rng(1).standard_normal(n)      # x given: the initial residual costs a product
    x, hist, it, mv, conv = model.bicgstabl(P, arrays, b, l=l, x=x0, max_mv_products=1)
    assert it == 0 and mv == 1 and not conv and np.array_equal(x, x0)
    x, hist, it, mv, conv = model.bicgstabl(P, arrays, b, l=l, x=x0, max_mv_products=2)
    assert it == 1 and mv == 1 + 2 * l


def test_zero_right_hand_side_tiny_sizes_and_breakdown(orc, model):
    """b = 0: no iteration, converged; n = 0 likewise; n = 1 solves in the first BiCG step and the minimal-residual system is
    0/0: NaN; diag(1, -1) with b = (1, 1): dot(rt, A*rt) = 0, Inf and NaN, no stop before max_mv_products"""
    arrays = csc_arrays(27, *convdiff_triplets(3, 3, 3, 2.0))
    for kind in KIND_NAMES:
        x, hist, it, mv, conv = model.bicgstabl(model.precon(kind, arrays, orc), arrays, np.zeros(27))
        assert it == 0 and mv == 0 and conv and list(hist) == [0.0] and not x.any()
    empty = (np.ones(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    x, hist, it, mv, conv = model.bicgstabl(model.precon("identity", empty, orc), empty, np.zeros(0))
    assert it == 0 and conv and list(hist) == [0.0] and len(x) == 0
    one = (np.array([1, 2], np.int64), np.array([1], np.int64), np.array([4.0]))
    x, hist, it, mv, conv = model.bicgstabl(model.precon("identity", one, orc), one, np.array([2.0]), l=1, max_mv_products=4)
    assert it == 2 and mv == 4 and not conv and hist[0] == 2.0 and np.isnan(hist[1:]).all() and np.isnan(x).all()
    D = (np.arange(1, 4, dtype=np.int64), np.array([1, 2], np.int64), np.array([1.0, -1.0]))
    x, hist, it, mv, conv = model.bicgstabl(model.precon("identity", D, orc), D, np.array([1.0, 1.0]), l=1, max_mv_products=8)
    assert it == 4 and mv == 8 and not conv and hist[0] == math.sqrt(2.0) and not np.isfinite(hist[1:]).any() and np.isnan(x).all()
