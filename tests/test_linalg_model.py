"""CPU: the model of tests/linalg_model.c pinned against scipy and numpy -- transpose bitwise against A.T.tocsc() (sorted indices),
issymmetric against np.array_equal(D, D.T) of the dense matrix, opnorm and the norms against np.linalg.norm within 1e-13 --
with stored zeros, -0.0, NaN and Inf among the values."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from linalg_modellib import Model, norm_exact, norm_ref


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("linalg_model_cpu"))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


SPECIAL = np.array([0.0, -0.0, 1.5, -2.0, np.inf, -np.inf, 3.0, -7.25], np.float64)
PAYLOAD_NAN = np.array([0x7FF800000000BEEF, 0xFFF8000000001234], np.uint64).view(np.float64)


def rand_csc(m, n, density, seed, vals=None):
    M = sp.random(m, n, density=density, format="csc", random_state=seed)
    M.sort_indices()
    nz = M.data - 0.5 if vals is None else vals(len(M.data))
    return (M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, np.ascontiguousarray(nz, np.float64))


def scipy_of(m, A):
    cp, rv, nz = A
    return sp.csc_matrix((nz.copy(), rv - 1, cp - 1), shape=(m, len(cp) - 1))


def dense(m, A):
    cp, rv, nz = A
    D = np.zeros((m, len(cp) - 1))
    for j in range(len(cp) - 1):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            D[rv[k] - 1, j] = nz[k]
    return D


def close(got, want):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want) or want == 0.0:
        return got == want
    return abs(got - want) <= 1e-13 * abs(want)


CASES = [(40, 30, 0.1, None), (1, 50, 0.4, None), (60, 1, 0.4, None), (35, 35, 0.15, lambda k: np.resize(SPECIAL, k)),
         (25, 45, 0.2, lambda k: np.resize(np.concatenate([SPECIAL, PAYLOAD_NAN]), k)), (20, 20, 0.0, None)]


@pytest.mark.parametrize("m,n,d,vals", CASES)
def test_transpose_against_scipy(model, m, n, d, vals):
    A = rand_csc(m, n, d, 1, vals)
    T = scipy_of(m, A).T.tocsc()
    T.sort_indices()
    cp, rv, nz = model.transpose(m, A)
    assert np.array_equal(cp, T.indptr + 1) and np.array_equal(rv, T.indices + 1)
    assert np.array_equal(bits(nz), bits(T.data))  # raw bits: -0.0 and NaN payloads moved as they are
    back = model.transpose(n, (cp, rv, nz))
    assert all(np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y) for x, y in zip(back, A))


@pytest.mark.parametrize("m,n,d,vals", CASES)
def test_mul_transpose_against_numpy(model, m, n, d, vals):
    A = rand_csc(m, n, d, 2, vals)
    x = np.random.default_rng(3).standard_normal(m)
    got = model.mul_transpose(A, x)
    D = dense(m, A)
    with np.errstate(invalid="ignore", over="ignore"):
        want = D.T @ x
        scale = np.abs(D.T) @ np.abs(x)
    for g, w, sc in zip(got, want, scale):
        if np.isfinite(w) and np.isfinite(sc):
            assert abs(g - w) <= 1e-12 * max(1.0, sc)
        elif np.isnan(w):
            assert math.isnan(g)
        else:
            assert g == w or math.isnan(g)


def test_mul_transpose_is_the_ordered_loop(model):
    """1e16 + 1 - 1e16 in stored order: the fold is not reassociated"""
    A = (np.array([1, 4]), np.array([1, 2, 3]), np.array([1e16, 1.0, -1e16]))
    assert model.mul_transpose(A, np.ones(3))[0] == 0.0
    assert model.mul_transpose((np.array([1, 4]), np.array([1, 2, 3]), np.array([1.0, 1e16, -1e16])), np.ones(3))[0] == 0.0
    assert model.mul_transpose((np.array([1, 4]), np.array([1, 2, 3]), np.array([1e16, -1e16, 1.0])), np.ones(3))[0] == 1.0


@pytest.mark.parametrize("m,n,d,vals", CASES)
def test_issymmetric_against_dense(model, m, n, d, vals):
    A = rand_csc(m, n, d, 4, vals)
    D = dense(m, A)
    assert model.issymmetric(m, A) == (D.shape[0] == D.shape[1] and np.array_equal(D, D.T))
    if m == n:  # a symmetric one from it
        S = sp.csc_matrix(scipy_of(m, A) + scipy_of(m, A).T)
        S.sort_indices()
        B = (S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64))
        Ds = dense(m, B)
        assert model.issymmetric(m, B) == np.array_equal(Ds, Ds.T)


def test_issymmetric_rules(model):
    cp = np.array([1, 3, 5, 6])
    rv = np.array([1, 2, 1, 2, 3])
    assert model.issymmetric(3, (cp, rv, np.array([1.0, 2.0, 2.0, 1.0, 5.0])))
    assert not model.issymmetric(3, (cp, rv, np.array([1.0, 2.0, 2.5, 1.0, 5.0])))
    assert not model.issymmetric(3, (cp, rv, np.array([np.nan, 2.0, 2.0, 1.0, 5.0])))
    assert model.issymmetric(3, (cp, rv, np.array([1.0, 0.0, -0.0, 1.0, 5.0])))
    assert model.issymmetric(3, (np.array([1, 3, 4, 5]), np.array([1, 3, 2, 3]), np.array([1.0, 0.0, 1.0, 5.0])))  # stored zero, no mirror


@pytest.mark.parametrize("m,n,d,vals", CASES)
def test_opnorm_general_against_numpy(model, m, n, d, vals):
    if m == 1 or n == 1:
        return
    A = rand_csc(m, n, d, 5, vals)
    D = dense(m, A)
    for p in (1, math.inf):
        with np.errstate(invalid="ignore"):
            want = float(np.linalg.norm(D, p))
        assert close(model.opnorm_general(m, A, p), want), p


@pytest.mark.parametrize("m,n,d,vals", CASES)
def test_norms_against_numpy(m, n, d, vals):
    nz = rand_csc(m, n, d, 6, vals)[2]
    for p in (math.inf, -math.inf, 0, 1, 2, 3, 0.5, -2.5):
        got = norm_ref(nz, p)
        if len(nz) == 0:
            assert got == 0.0
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            want = float(np.linalg.norm(nz, p))
        if np.isnan(nz).any() and p != 0:
            assert math.isnan(got)
        else:
            assert close(got, want), (p, got, want)
    for p in (math.inf, -math.inf, 0):
        assert norm_exact(nz, p) == norm_ref(nz, p) or math.isnan(norm_ref(nz, p))


def test_norm2_without_overflow():
    for s in (1e200, 1e-200):
        v = s * np.random.default_rng(7).standard_normal(1000)
        want = s * math.sqrt(math.fsum(((v / s) ** 2).tolist()))
        assert close(norm_ref(v, 2), want) and math.isfinite(want) and want > 0
