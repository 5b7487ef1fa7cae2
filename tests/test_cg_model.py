"""CPU: the model of preconditioned conjugate gradients (tests/cg_model.c) the GPU tests compare esp_cg with bit for bit.
It converges with every preconditioner on the reference's own test matrices and meets the reference's acceptance
(test_block.jl:14-36: `sol ≈ ones`); scipy's cg with the same preconditioner reaches the same solution; the fixed summation
shape stays within the derivable error bound of an exact sum."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cg_modellib import RELTOL, Model

KIND_NAMES = ["identity", "jacobi", "ilu0", "iluam"]
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("cg_model"))


def isapprox(x, y):
    """Julia's x ≈ y for vectors: norm(x - y) <= sqrt(eps) * max(norm(x), norm(y))"""
    return np.linalg.norm(x - y) <= math.sqrt(EPS) * max(np.linalg.norm(x), np.linalg.norm(y))


def fdrand_arrays(orc, *dims):
    """copies of the CSC arrays of the oracle's fdrand(dims...) (the arrays themselves live only as long as the matrix)"""
    O = orc.fdrand(*dims)
    return tuple(np.array(a, copy=True) for a in O.sparse().arrays())


MATRICES = {"fdrand20": (20, 20, 20), "fdrand100x100": (100, 100)}


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("matrix", ["fdrand20", "fdrand100x100"])
def test_model_converges_like_the_reference(orc, model, kind, matrix):
    """test_block.jl:14-36: b = A*ones, sol = cg(A, b, Pl = ...), sol ≈ ones -- and scipy's cg agrees"""
    arrays = fdrand_arrays(orc, *MATRICES[matrix])
    cp, rv, nz = arrays
    n = len(cp) - 1
    ones = np.ones(n)
    b = model.mul(arrays, ones)
    P = model.precon(kind, arrays, orc)
    x, hist, it, conv = model.cg(P, arrays, b)
    assert conv and it < n and len(hist) == it + 1
    assert hist[-1] <= RELTOL * hist[0]
    assert isapprox(x, ones)
    S = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).tocsr()
    count = [0]

    def tick(_):
        count[0] += 1

    M = spla.LinearOperator((n, n), matvec=lambda v: model.ldiv(P, arrays, v), dtype=np.float64)
    xs, info = spla.cg(S, b, rtol=RELTOL, atol=0.0, maxiter=n, M=M, callback=tick)
    print("%s %s: model %d iterations, scipy %d; |x - 1|/sqrt(n) = %.3e (model) %.3e (scipy)"
          % (matrix, kind, it, count[0], np.linalg.norm(x - ones) / math.sqrt(n), np.linalg.norm(xs - ones) / math.sqrt(n)))
    assert info == 0
    assert isapprox(xs, ones) and isapprox(xs, x)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1000, 65536, 65537, 200003])
def test_ordered_dot_within_the_bound_of_an_exact_sum(model, n):
    """any order of summation of n products errs by at most (n - 1) eps sum|a_i b_i| to first order (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2; the products themselves add eps/2 each): n eps sum|a_i b_i| holds both"""
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    b = rng.standard_normal(n)
    got = model.dot(a, b)
    exact = math.fsum(float(x) * float(y) for x, y in zip(a, b))   # (the rounded products summed exactly)
    bound = n * EPS * math.fsum(abs(float(x) * float(y)) for x, y in zip(a, b))
    print("n = %d: |dot - fsum| = %.3e, bound %.3e" % (n, abs(got - exact), bound))
    assert abs(got - exact) <= bound
    if n == 0:
        assert got == 0.0 and not math.copysign(1.0, got) < 0
    if n == 1:
        assert got == 0.0 + a[0] * b[0]


def test_dot_shape_by_hand(model):
    """the shape at a size that is no multiple of 256, rebuilt with NumPy: chunk trees, group trees, strided sums, last tree"""
    n = 3 * 65536 + 700
    rng = np.random.default_rng(12)
    a, b = rng.standard_normal(n), rng.standard_normal(n)

    def tree(v):   # rows of 256 -> one value per row, s[t] = s[t] + s[t + w]
        v = v.copy()
        for w in (128, 64, 32, 16, 8, 4, 2, 1):
            v[:, :w] = v[:, :w] + v[:, w:2 * w]
        return v[:, 0].copy()

    def level(v):
        pad = np.zeros((len(v) + 255) // 256 * 256)
        pad[:len(v)] = v
        return tree(pad.reshape(-1, 256))

    p1 = level(level(a * b))
    lanes = np.zeros(256)
    for q in range(len(p1)):   # lane q % 256 adds its values in increasing q
        lanes[q % 256] = lanes[q % 256] + p1[q]
    want = tree(lanes.reshape(1, 256))[0]
    assert model.dot(a, b) == want


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_zero_right_hand_side(orc, model, kind):
    """b = 0: residual 0 <= tol 0 -- no iteration, x untouched, converged"""
    arrays = fdrand_arrays(orc, 6, 5, 4)
    n = len(arrays[0]) - 1
    P = model.precon(kind, arrays, orc)
    x, hist, it, conv = model.cg(P, arrays, np.zeros(n))
    assert it == 0 and conv and list(hist) == [0.0] and not x.any()


def test_tiny_sizes(orc, model):
    """n = 0: nothing to do; n = 1: one step solves a*x = b"""
    empty = (np.ones(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    x, hist, it, conv = model.cg(model.precon("identity", empty, orc), empty, np.zeros(0))
    assert it == 0 and conv and list(hist) == [0.0] and len(x) == 0
    one = (np.array([1, 2], np.int64), np.array([1], np.int64), np.array([4.0]))
    for kind in KIND_NAMES:
        x, hist, it, conv = model.cg(model.precon(kind, one, orc), one, np.array([2.0]))
        assert it == 1 and conv and x[0] == 0.5 and hist[0] == 2.0 and hist[1] == 0.0


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_size_off_the_chunk(orc, model, kind):
    """n = 7*11*13 = 1001 (no multiple of 256), cg! from a random start.  What the loop promises is its stopping test on the
    recurrence residual, not an error bound (a random start is far from the solution, so sqrt(eps) of ITS residual says little
    about |x - 1|); the true residual b - A*x differs from the recurrence's by accumulated rounding only, orders below
    sqrt(eps)*|r0|: a factor 2 holds it."""
    arrays = fdrand_arrays(orc, 7, 11, 13)
    n = len(arrays[0]) - 1
    rng = np.random.default_rng(3)
    b = model.mul(arrays, np.ones(n))
    x, hist, it, conv = model.cg(model.precon(kind, arrays, orc), arrays, b, x=rng.standard_normal(n))
    assert conv and 0 < it < n and hist[-1] <= RELTOL * hist[0]
    assert np.linalg.norm(b - model.mul(arrays, x)) <= 2 * RELTOL * hist[0]


def test_truncation_and_breakdown(orc, model):
    """maxiter cuts the loop (not converged); an indefinite diagonal gives dot(u, c) = 0 in the first step: alpha = Inf, the residual
    norm Inf after it and NaN from then on, no stop before maxiter"""
    arrays = fdrand_arrays(orc, 10, 10, 10)
    n = len(arrays[0]) - 1
    b = model.mul(arrays, np.ones(n))
    P = model.precon("jacobi", arrays, orc)
    _, full, _, _ = model.cg(P, arrays, b)
    for k in (1, 2, 7):
        x, hist, it, conv = model.cg(P, arrays, b, maxiter=k)
        assert it == k and not conv and np.array_equal(hist, full[:k + 1])
    D = (np.arange(1, 4, dtype=np.int64), np.array([1, 2], np.int64), np.array([1.0, -1.0]))
    x, hist, it, conv = model.cg(model.precon("identity", D, orc), D, np.array([1.0, 1.0]), maxiter=4)
    assert it == 4 and not conv and hist[0] == math.sqrt(2.0) and np.isinf(hist[1]) and np.isnan(hist[2:]).all() and np.isnan(x).all()
