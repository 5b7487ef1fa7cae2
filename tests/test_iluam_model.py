"""CPU: the independent model of ILUAMPreconditioner (tests/iluam_model.c) is held to account -- its level-ordered entry
points equal its literal loops bit for bit (the argument the device's level scheduling rests on), the literal loops are
pinned on a case where ILU(0) is plain LU and satisfy ILU(0)'s defining property to the standard rounding bound -- and
the new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from iluam_modellib import Model, level_order, level_schedules
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("iluam_model"))


def nonsymmetric_csc(n=3000, extra=20000, seed=5):
    """the construction of nonsymmetric() in test_precon_gpu.py on the host: a non-symmetric, diagonally dominant matrix with
    a random extra pattern, every diagonal stored (duplicates summed)"""
    rng = np.random.default_rng(seed)
    d = np.arange(n)
    I, J, V = [d], [d], [20.0 + rng.random(n)]
    i = rng.integers(0, n, extra)
    I.append(i)
    J.append(np.clip(i + rng.integers(-400, 400, extra), 0, n - 1))
    V.append(rng.standard_normal(extra))
    I.append(rng.integers(0, n, 2000))
    J.append(rng.integers(0, n, 2000))
    V.append(rng.standard_normal(2000))
    A = sp.coo_matrix((np.concatenate(V), (np.concatenate(I), np.concatenate(J))), shape=(n, n)).tocsc()
    A.sort_indices()
    return A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.copy()


@pytest.mark.parametrize("matrix", ["fdrand12", "nonsymmetric"])
def test_level_order_equals_literal_loops(model, orc, matrix):
    """(a) the factorization run level by level with the columns of a level in REVERSE, and the two solves as row gathers
    in level order (rows of a level reversed too), are bitwise the sequential loops."""
    if matrix == "fdrand12":
        O = orc.fdrand(12, 12, 12, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
        cp, rv, nz = (np.array(a) for a in O.sparse().arrays())
    else:
        cp, rv, nz = nonsymmetric_csc()
    n = len(cp) - 1
    lc, lf, lb = level_schedules(cp, rv)
    if matrix == "fdrand12":
        assert (lc.max() + 1, lf.max() + 1, lb.max() + 1) == (34, 34, 34)   # nx + ny + nz - 2
    f, diag = model.factor((cp, rv, nz))
    f2, diag2 = model.factor((cp, rv, nz), order=level_order(lc, reverse_inside=True))
    assert np.array_equal(diag, diag2) and np.array_equal(bits(f), bits(f2))
    assert np.all(np.isfinite(f))
    v = np.random.default_rng(1).standard_normal(n)
    x = model.ldiv((cp, rv, nz), f, diag, v)
    x2 = model.ldiv((cp, rv, nz), f, diag, v, fwd=level_order(lf, True), bwd=level_order(lb, True))
    assert np.array_equal(bits(x), bits(x2))
    x3 = model.ldiv((cp, rv, nz), f, diag, v, inplace=True)      # ldiv!(ILU, b)
    assert np.array_equal(bits(x), bits(x3))


def split_factor(cp, rv, f, dtype=np.longdouble):
    """dense unit-lower L and upper U from the factorization's values"""
    n = len(cp) - 1
    cols = np.repeat(np.arange(n), np.diff(cp))
    rows = rv - 1
    L = np.eye(n, dtype=dtype)
    U = np.zeros((n, n), dtype=dtype)
    lo = rows > cols
    L[rows[lo], cols[lo]] = f[lo]
    U[rows[~lo], cols[~lo]] = f[~lo]
    return L, U, rows, cols


def test_dense_pattern_is_plain_lu(model):
    """(b) pinned: on a dense 6x6 pattern ILU(0) is LU.  A = L0*U0 with small integers and power-of-two pivots, so every
    operation of iluAM and of ldiv! is exact: the factor IS (L0, U0) and ldiv! solves A x = b exactly."""
    n = 6
    rng = np.random.default_rng(12)
    L0 = np.tril(rng.integers(-3, 4, (n, n)).astype(np.float64), -1) + np.eye(n)
    U0 = np.triu(rng.integers(-3, 4, (n, n)).astype(np.float64), 1) + np.diag([2.0, -4.0, 1.0, 8.0, -2.0, 4.0])
    A = L0 @ U0
    cp = np.arange(0, n * n + 1, n, dtype=np.int64) + 1
    rv = np.tile(np.arange(1, n + 1, dtype=np.int64), n)
    nz = np.ascontiguousarray(A.T).ravel()          # column-major
    f, diag = model.factor((cp, rv, nz))
    assert list(diag) == [j * n + j + 1 for j in range(n)]
    L, U, _, _ = split_factor(cp, rv, f, np.float64)
    assert np.array_equal(L, L0) and np.array_equal(U, U0)
    x0 = rng.integers(-5, 6, n).astype(np.float64) * 4.0
    assert np.array_equal(model.ldiv((cp, rv, nz), f, diag, A @ x0), x0)


def test_ilu0_defining_property(model, orc):
    """(b) property: on every stored position |(L*U - A)_ij| <= gamma_k (|L||U|)_ij, gamma_k = k eps/(1 - k eps) with eps the
    unit roundoff 2^-53 and k = the entry's number of terms + 2 (the division and the final subtraction) -- the standard
    bound of a k-term inner product, not a tuned number.  L*U is formed in np.longdouble."""
    O = orc.fdrand(8, 8, 8, rand_mode=1, seed=0x5EED0002, style=orc.KIND_UPDATE)
    cp, rv, nz = (np.array(a) for a in O.sparse().arrays())
    f, _ = model.factor((cp, rv, nz))
    L, U, rows, cols = split_factor(cp, rv, f)
    LU = L @ U
    absLU = np.abs(L) @ np.abs(U)
    terms = (L != 0).astype(np.int64) @ (U != 0).astype(np.int64)
    eps = np.longdouble(2.0) ** -53
    k = (terms[rows, cols] + 2).astype(np.longdouble)
    gamma = k * eps / (1 - k * eps)
    err = np.abs(LU[rows, cols] - nz.astype(np.longdouble))
    bound = gamma * absLU[rows, cols]
    print("largest error/bound: %.3f, most terms: %d" % (float((err / bound).max()), int(terms[rows, cols].max())))
    assert np.all(err <= bound)
    # ... and it is an approximate inverse: one application reduces the residual of A x = v
    n = len(cp) - 1
    v = np.random.default_rng(3).standard_normal(n)
    x = model.ldiv((cp, rv, nz), f, model.factor((cp, rv, nz))[1], v)
    A = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))
    assert np.linalg.norm(A @ x - v) < np.linalg.norm(v)


def test_iluam_entry_points_declared_and_exported(esp):
    """(c) the header declares the constant and the two read-only calls; the package exports the class."""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_ILUAM\s+2\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\besp_precon_get_factor\s*\(", code) and re.search(r"\besp_precon_levels\s*\(", code)
    lib = esp._lib.load()
    assert hasattr(lib, "esp_precon_get_factor") and hasattr(lib, "esp_precon_levels")
    assert esp.ESP_PRECON_ILUAM == 2
    assert (esp.ESP_PRECON_JACOBI, esp.ESP_PRECON_ILU0) == (0, 1)
    assert issubclass(esp.ILUAMPreconditioner, object) and esp.ILUAMPreconditioner.KIND == 2
    with pytest.raises(TypeError):
        esp.ILUAMPreconditioner("not a matrix")
