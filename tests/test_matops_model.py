"""CPU: the independent model of the device matrix algebra (tests/matops_model.c) agrees with scipy on patterns and, to rounding,
on values; it keeps the reference's rules (a leading -0.0 product assigned, A - A empty); and the library exports the new
entry points."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from matops_modellib import OP_ADD, OP_SUB, Model
from refmodel import bits


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("matops_model"))


def rand_csc(m, n, density, seed):
    M = sp.random(m, n, density=density, format="csc", random_state=seed)
    M.sort_indices()
    return (M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, M.data.astype(np.float64))


def to_scipy(m, csc):
    cp, rv, nz = csc
    return sp.csc_matrix((nz, rv - 1, cp - 1), shape=(m, len(cp) - 1))


@pytest.mark.parametrize("m,k,n,d", [(30, 40, 20, 0.1), (200, 150, 170, 0.03), (1, 5, 7, 0.5), (50, 50, 50, 0.0)])
def test_matmul_matches_scipy(model, m, k, n, d):
    A, B = rand_csc(m, k, d, 1), rand_csc(k, n, d, 2)
    cp, rv, nz = model.matmul(m, A, B)
    want = to_scipy(m, A) @ to_scipy(k, B)
    want.sort_indices()
    # scipy stores every reached row too (no dropping of computed zeros in its SpGEMM)
    assert np.array_equal(cp - 1, want.indptr) and np.array_equal(rv - 1, want.indices)
    assert np.allclose(nz, want.data, rtol=1e-13, atol=0)


def test_matmul_first_product_assigned(model):
    """-0.0 as the only product stays -0.0 (0.0 + -0.0 would give +0.0); a later product is added to it"""
    A = (np.array([1, 2, 3]), np.array([1, 1]), np.array([-1.0, 1.0]))       # 1 x 2: A[1,1] = -1, A[1,2] = 1
    B = (np.array([1, 2, 4]), np.array([1, 1, 2]), np.array([0.0, 0.0, 2.0]))  # 2 x 2: B[1,1] = 0; B[1,2] = 0, B[2,2] = 2
    cp, rv, nz = model.matmul(1, A, B)
    assert list(cp) == [1, 2, 3] and list(rv) == [1, 1]
    assert bits(nz)[0] == bits(np.array([-0.0]))[0]
    assert nz[1] == 2.0


@pytest.mark.parametrize("op", [OP_ADD, OP_SUB])
def test_add_matches_scipy(model, op):
    A, B = rand_csc(60, 70, 0.08, 3), rand_csc(60, 70, 0.08, 4)
    cp, rv, nz = model.add(A, B, op)
    want = to_scipy(60, A) + to_scipy(60, B) if op == OP_ADD else to_scipy(60, A) - to_scipy(60, B)
    want.eliminate_zeros()
    want.sort_indices()
    assert np.array_equal(cp - 1, want.indptr) and np.array_equal(rv - 1, want.indices)
    assert np.allclose(nz, want.data, rtol=1e-15, atol=0)


def test_add_drops_zero_results(model):
    A = rand_csc(40, 30, 0.2, 5)
    cp, rv, nz = model.add(A, A, OP_SUB)
    assert len(rv) == 0 and np.all(cp == 1)
    # a stored -0.0 + 0.0 compares == 0 and goes as well; NaN stays
    Z = (np.array([1, 3]), np.array([1, 2]), np.array([-0.0, np.nan]))
    cp, rv, nz = model.add(Z, (np.array([1, 1]), np.array([], np.int64), np.array([])), OP_ADD)
    assert list(rv) == [2] and np.isnan(nz[0])


def test_diag_scale_keeps_pattern(model):
    A = rand_csc(20, 25, 0.2, 6)
    A[2][::3] = 0.0
    d = np.random.default_rng(0).standard_normal(20)
    cp, rv, nz = model.diag_scale(A, d, 0)
    assert np.array_equal(cp, A[0]) and np.array_equal(rv, A[1])
    assert np.allclose(to_scipy(20, (cp, rv, nz)).toarray(), np.diag(d) @ to_scipy(20, A).toarray(), rtol=1e-15, atol=0)
    e = np.random.default_rng(1).standard_normal(25)
    _, _, nz = model.diag_scale(A, e, 1)
    assert np.allclose(to_scipy(20, (cp, rv, nz)).toarray(), to_scipy(20, A).toarray() @ np.diag(e), rtol=1e-15, atol=0)


def test_library_exports_matops(esp):
    lib = ctypes.CDLL(esp.library_path())
    for name in ("esp_matmul", "esp_add", "esp_diag_scale", "esp_debug_matmul_tier"):
        assert hasattr(lib, name), name
    assert hasattr(esp, "Diagonal")
    for op in ("__mul__", "__add__", "__sub__", "__radd__", "__rsub__"):
        assert op in vars(esp.ExtendableSparseMatrix), op
