"""GPU: the algebra of assembled matrices on the device CSC (include/esparse_hip.h: esp_matmul, esp_add, esp_diag_scale) against
the independent model of tests/matops_model.c -- bitwise on colptr, rowval and nzval."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from matops_modellib import OP_ADD, OP_SUB, Model
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_STATE = -1, -6
CANON_NAN = np.uint64(0x7FF8000000000000)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("matops_model"))


def canon(nz):
    """the bits of nzval with every NaN as one quiet NaN (the payload of a NaN that an operation creates is the platform's)"""
    b = bits(nz).copy()
    b[np.isnan(nz)] = CANON_NAN
    return b


def arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def assert_same(got, want, what=""):
    (cp1, rv1, nz1), (cp2, rv2, nz2) = got, want
    assert np.array_equal(cp1, cp2), what + " colptr differs"
    assert np.array_equal(rv1, rv2), what + " rowval differs"
    assert np.array_equal(canon(nz1), canon(nz2)), what + " nzval differs (bitwise)"


def rand_csc(m, n, density, seed, values=None):
    M = sp.random(m, n, density=density, format="csc", random_state=seed)
    M.sort_indices()
    nz = M.data.astype(np.float64) - 0.5 if values is None else values(len(M.data))
    return (M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, np.ascontiguousarray(nz, np.float64))


def ext(esp, m, csc):
    cp, rv, nz = csc
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(m, len(cp) - 1, cp, rv, nz))


def check_matmul(esp, model, A, B, tier=0):
    C = A.matmul(B, tier=tier)
    want = model.matmul(A.m, arrays(A), arrays(B))
    assert isinstance(C, esp.ExtendableSparseMatrix) and C.shape == (A.m, B.n) and C.nnznew() == 0
    assert_same(arrays(C), want, "A*B")
    return C, want


def nonsymmetric(esp):
    from test_precon_gpu import nonsymmetric as ns
    return ns(esp)


# ---- A*B ----------------------------------------------------------------------------------------------------------------
def test_matmul_fdrand40_squared(esp, model):
    A = esp.fdrand(40, 40, 40, rand_mode=1, seed=11)
    check_matmul(esp, model, A, A)  # aliased operands


@pytest.mark.parametrize("m,k,n,d", [(300, 200, 250, 0.02), (1, 40, 3, 0.5), (500, 7, 600, 0.3), (64, 64, 1, 0.5)])
def test_matmul_rectangular(esp, model, m, k, n, d):
    check_matmul(esp, model, ext(esp, m, rand_csc(m, k, d, 1)), ext(esp, k, rand_csc(k, n, d, 2)))


def test_matmul_nonsymmetric(esp, model):
    A = nonsymmetric(esp)
    B = ext(esp, A.n, rand_csc(A.n, 500, 0.01, 3))
    check_matmul(esp, model, A, A)
    check_matmul(esp, model, A, B)


def test_matmul_empty_columns_and_zero_matrix(esp, model):
    A = rand_csc(80, 90, 0.05, 4)
    cp, rv, nz = A
    keep = np.diff(cp) > 0
    keep[::3] = False  # every third column of A empty
    M = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(80, 90))
    M = M @ sp.diags(keep.astype(float))
    M.eliminate_zeros()
    M.sort_indices()
    Ae = ext(esp, 80, (M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, M.data.astype(np.float64)))
    B = rand_csc(90, 70, 0.05, 5)
    cpb = B[0].copy()
    Be = ext(esp, 90, B)
    check_matmul(esp, model, Ae, Be)
    Z = esp.ExtendableSparseMatrix(80, 90)
    C, want = check_matmul(esp, model, Z, Be)
    assert C.nnz() == 0
    check_matmul(esp, model, Ae, esp.ExtendableSparseMatrix(90, 70))
    assert np.any(np.diff(cpb) == 0)


@pytest.mark.parametrize("tier", [0, 1, 2])
def test_matmul_stored_zeros_and_negative_zero(esp, model, tier):
    """explicitly stored zeros stay, a -0.0 first product is assigned (not 0.0 + -0.0) -- in either tier"""
    vals = lambda k: np.resize(np.array([0.0, -0.0, 1.5, -2.0, 0.0, 3.0]), k)
    A = ext(esp, 60, rand_csc(60, 60, 0.1, 6, vals))
    B = ext(esp, 60, rand_csc(60, 60, 0.1, 7, vals))
    C, want = check_matmul(esp, model, A, B, tier=tier)
    assert np.any(bits(want[2]) == bits(np.array([-0.0]))[0]) and np.any(want[2] == 0.0)


def test_matmul_inf_nan(esp, model):
    vals = lambda k: np.resize(np.array([np.inf, 1.0, -np.inf, np.nan, 0.0, 2.0, -1.0]), k)
    check_matmul(esp, model, ext(esp, 50, rand_csc(50, 50, 0.15, 8, vals)), ext(esp, 50, rand_csc(50, 50, 0.15, 9, vals)))


def dense_column_case(esp):
    """B's first column is dense: its product count (nnz(A)) is far above the fused tier's cap; the others are short"""
    k = 3000
    A = ext(esp, 2500, rand_csc(2500, k, 0.004, 10))
    Bs = sp.random(k, 400, density=0.002, format="csc", random_state=11)
    Bs = sp.csc_matrix(Bs)
    Bs[:, 0] = np.random.default_rng(12).standard_normal((k, 1))
    Bs.sort_indices()
    B = ext(esp, k, (Bs.indptr.astype(np.int64) + 1, Bs.indices.astype(np.int64) + 1, Bs.data.astype(np.float64)))
    assert A.nnz() > 4 * 2048
    return A, B


def test_matmul_both_tiers_in_one_product(esp, model):
    A, B = dense_column_case(esp)
    C0, want = check_matmul(esp, model, A, B)
    C1, _ = check_matmul(esp, model, A, B, tier=1)
    C2, _ = check_matmul(esp, model, A, B, tier=2)
    assert_same(arrays(C1), arrays(C2), "fused vs generic")


def bin_edge_case(esp, counts, m=3000, seed=90):
    """A (m x 128): column j has 1 + (j-1) % 64 stored rows; B column i picks A columns whose lengths sum to counts[i] exactly,
    so column i of A*B has exactly counts[i] products (random rows: some fold, most stay distinct)"""
    rng = np.random.default_rng(seed)
    lens = np.array([1 + (j % 64) for j in range(128)])
    cpA = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int64)
    rvA = np.concatenate([np.sort(rng.choice(m, L, replace=False)) + 1 for L in lens]).astype(np.int64)
    nzA = rng.standard_normal(len(rvA))
    order = np.argsort(-lens, kind="stable")
    cols, rvB = [1], []
    for t in counts:
        pick, left = [], t
        for j in order:
            if lens[j] <= left:
                pick.append(j)
                left -= lens[j]
        assert left == 0, t
        rvB.extend(sorted(j + 1 for j in pick))
        cols.append(len(rvB) + 1)
    rvB = np.array(rvB, np.int64)
    A = ext(esp, m, (cpA, rvA, nzA))
    B = ext(esp, 128, (np.array(cols, np.int64), rvB, rng.standard_normal(len(rvB))))
    return A, B


def test_matmul_fused_bin_edges(esp, model):
    """columns of 1900..2049 products: weight above a bin (bins left empty), a bin of 1918 + 2048 = 3966 products (the
    4096-key sort, every sequence bit), the cap exactly (2048: fused) and one above (2049: generic), next to tiny and empty
    columns; automatic, fused and generic tiers agree bitwise with the model and with each other"""
    counts = [1918, 2048, 1919, 2048, 2047, 1921, 1900, 5, 2049, 3000, 1, 0, 2048, 1920, 1950, 1, 1, 2000, 0, 4096, 7, 1999]
    A, B = bin_edge_case(esp, counts)
    got = [arrays(check_matmul(esp, model, A, B, tier=t)[0]) for t in (0, 1, 2)]
    assert_same(got[0], got[1], "automatic vs fused")
    assert_same(got[1], got[2], "fused vs generic")


@pytest.mark.parametrize("tier", [1, 2])
def test_matmul_forced_tier_fdrand(esp, model, tier):
    A = esp.fdrand(24, 24, 24, rand_mode=1, seed=13)
    check_matmul(esp, model, A, A, tier=tier)


def test_matmul_size_128(esp, model):
    A = esp.fdrand(128, 128, 128, rand_mode=1, seed=0x5EED0002)
    check_matmul(esp, model, A, A)


# ---- A+B, A-B -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["+", "-"])
@pytest.mark.parametrize("pattern", ["equal", "overlap", "disjoint"])
def test_add_sub(esp, model, op, pattern):
    m, n = 400, 300
    A = rand_csc(m, n, 0.03, 20)
    if pattern == "equal":
        B = (A[0], A[1], np.random.default_rng(21).standard_normal(len(A[2])))
    elif pattern == "overlap":
        B = rand_csc(m, n, 0.03, 22)
    else:  # A in the odd rows, B in the even ones
        Ms = sp.csc_matrix((A[2], A[1] - 1, A[0] - 1), shape=(m, n))
        Ma = sp.csc_matrix(Ms.multiply(np.tile((np.arange(m) % 2 == 0)[:, None], (1, n))))
        Mb = sp.csc_matrix(sp.random(m, n, density=0.03, format="csc", random_state=23).multiply(np.tile((np.arange(m) % 2 == 1)[:, None], (1, n))))
        for M in (Ma, Mb):
            M.eliminate_zeros()
            M.sort_indices()
        A = (Ma.indptr.astype(np.int64) + 1, Ma.indices.astype(np.int64) + 1, Ma.data.astype(np.float64))
        B = (Mb.indptr.astype(np.int64) + 1, Mb.indices.astype(np.int64) + 1, Mb.data.astype(np.float64))
    Ae, Be = ext(esp, m, A), ext(esp, m, B)
    C = Ae + Be if op == "+" else Ae - Be
    assert isinstance(C, esp.ExtendableSparseMatrix)
    assert_same(arrays(C), model.add(A, B, OP_ADD if op == "+" else OP_SUB), "A%sB" % op)


def test_add_fdrand_and_aliased(esp, model):
    A = esp.fdrand(40, 40, 40, rand_mode=1, seed=14)
    a = arrays(A)
    assert_same(arrays(A + A), model.add(a, a, OP_ADD), "A+A")
    D = A - A
    assert D.nnz() == 0 and np.all(arrays(D)[0] == 1)


def test_add_cancellation_inside_a_column(esp, model):
    """rows whose sum cancels are dropped, exactly those"""
    A = (np.array([1, 6]), np.array([1, 2, 3, 4, 5]), np.array([1.0, 2.0, 3.0, -0.0, 5.0]))
    B = (np.array([1, 6]), np.array([1, 2, 3, 4, 6]), np.array([-1.0, 0.5, -3.0, 0.0, 7.0]))
    C = ext(esp, 6, A) + ext(esp, 6, B)
    cp, rv, nz = arrays(C)
    assert list(rv) == [2, 5, 6] and list(nz) == [2.5, 5.0, 7.0]
    assert_same((cp, rv, nz), model.add(A, B, OP_ADD))


def test_add_long_columns(esp, model):
    """dense columns: a merge tile lies inside one column, pairs split by tile borders"""
    m = 5000
    A = rand_csc(m, 4, 0.9, 24)
    B = rand_csc(m, 4, 0.9, 25)
    for op, o in (("+", OP_ADD), ("-", OP_SUB)):
        C = ext(esp, m, A) + ext(esp, m, B) if op == "+" else ext(esp, m, A) - ext(esp, m, B)
        assert_same(arrays(C), model.add(A, B, o), "long columns " + op)


# ---- Diagonal scaling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("inplace", [False, True])
def test_diag_scale(esp, model, side, where, inplace):
    m, n = 700, 500
    vals = lambda k: np.resize(np.array([0.0, 1.5, -2.0, 3.0, -0.0]), k)
    A = rand_csc(m, n, 0.02, 30, vals)
    d = np.random.default_rng(31).standard_normal(m if side == "left" else n)
    d[::7] = 0.0
    want = model.diag_scale(A, d, 0 if side == "left" else 1)
    Ae = ext(esp, m, A)
    dd = d
    if where == "torch":
        import torch
        dd = torch.tensor(d, dtype=torch.float64, device="cuda")
    if inplace:
        R = Ae.diag_scale(dd, side=side, inplace=True)
        assert R is Ae
    else:
        R = esp.Diagonal(dd) * Ae if side == "left" else Ae * esp.Diagonal(dd)
        assert R is not Ae and isinstance(R, esp.ExtendableSparseMatrix)
        assert_same(arrays(Ae), A, "the operand")
    got = arrays(R)
    assert np.array_equal(got[0], A[0]) and np.array_equal(got[1], A[1])  # the pattern of A, zeros included
    assert_same(got, want, "diag scale")


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_errors(esp):
    lib = esp._lib.load()
    A = ext(esp, 30, rand_csc(30, 20, 0.2, 40))
    B = ext(esp, 20, rand_csc(20, 25, 0.2, 41))
    C = esp.ExtendableSparseMatrix(30, 25)
    z = ctypes.c_int64()
    A.updateindex("+", 1.0, 1, 1)
    A._d.commit()
    assert lib.esp_matmul(A._d.h, B._d.h, C._d.h, ctypes.byref(z)) == ESP_ERR_STATE
    S = esp.ExtendableSparseMatrix(30, 20)
    assert lib.esp_add(A._d.h, S._d.h, 0, esp.ExtendableSparseMatrix(30, 20)._d.h, ctypes.byref(z)) == ESP_ERR_STATE
    A.flush()
    assert lib.esp_matmul(B._d.h, A._d.h, esp.ExtendableSparseMatrix(20, 20)._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    assert lib.esp_add(A._d.h, B._d.h, 0, esp.ExtendableSparseMatrix(30, 20)._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    Q = ext(esp, 20, rand_csc(20, 20, 0.2, 42))
    assert lib.esp_matmul(Q._d.h, Q._d.h, Q._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    assert lib.esp_add(A._d.h, S._d.h, 0, A._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    assert lib.esp_add(A._d.h, S._d.h, 0, S._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    with pytest.raises(ValueError, match="DimensionMismatch"):
        B * A
    with pytest.raises(ValueError, match="DimensionMismatch"):
        A + B
    # a refused call leaves c as it was
    assert C.nnz() == 0


# ---- results are live matrices ------------------------------------------------------------------------------------------
def test_result_updates_and_flush(esp, orc, model):
    A = ext(esp, 200, rand_csc(200, 150, 0.03, 50))
    B = ext(esp, 150, rand_csc(150, 180, 0.03, 51))
    C = A * B
    cp, rv, nz = model.matmul(200, arrays(A), arrays(B))
    O = orc.ExtendableSparseMatrix(orc.CSC(200, 180, cp, rv, nz))
    rng = np.random.default_rng(52)
    J = np.repeat(np.arange(1, 181), np.diff(cp))
    stored = rng.integers(0, len(rv), 300)
    I = np.concatenate([rv[stored], rng.integers(1, 201, 300)])
    Jc = np.concatenate([J[stored], rng.integers(1, 181, 300)])
    V = rng.standard_normal(600)
    for i, j, v in zip(I, Jc, V):
        C.updateindex("+", v, int(i), int(j))
        O.updateindex(orc.OP_ADD, v, int(i), int(j))
    C.flush()
    O.flush()
    assert_same(arrays(C), O.arrays(), "C after updates")


def test_result_pattern_hash_and_precon(esp, model):
    A = ext(esp, 300, rand_csc(300, 300, 0.02, 60))
    B = ext(esp, 300, rand_csc(300, 300, 0.02, 61))
    C = A * B
    cp, rv, nz = arrays(C)
    assert C.phash == esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(300, 300, cp, rv, nz)).phash
    S = A + B
    assert S.phash == esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(300, 300, *arrays(S))).phash
    n = 300
    d = np.arange(1, n + 1)
    E = esp.ExtendableSparseMatrix(n, n)
    E.append(esp.ESP_UPDATE, d, d, 10.0 + np.random.default_rng(62).random(n))
    E.flush()
    P = esp.JacobiPreconditioner(E + B)
    u = P.ldiv(np.ones(n))
    assert np.all(np.isfinite(u))


# ---- the reference's test_operations.jl ---------------------------------------------------------------------------------
def test_reference_operations(esp, model):
    for seed in range(5):
        Ah, Bh = rand_csc(10, 10, 0.1, 70 + seed), rand_csc(10, 10, 0.1, 80 + seed)
        A = esp.SparseMatrixCSC(10, 10, *Ah)
        B = esp.SparseMatrixCSC(10, 10, *Bh)
        extA, extB = esp.ExtendableSparseMatrix(A), esp.ExtendableSparseMatrix(B)
        for got, want in ((A + extB, model.add(Ah, Bh, OP_ADD)), (A - extB, model.add(Ah, Bh, OP_SUB)),
                          (extA + B, model.add(Ah, Bh, OP_ADD)), (extA - B, model.add(Ah, Bh, OP_SUB))):
            assert isinstance(got, esp.SparseMatrixCSC)
            assert_same(got.arrays(), want)
        for got, want in ((extA * extB, model.matmul(10, Ah, Bh)), (extA + extB, model.add(Ah, Bh, OP_ADD)),
                          (extA - extB, model.add(Ah, Bh, OP_SUB))):
            assert isinstance(got, esp.ExtendableSparseMatrix)
            assert_same(arrays(got), arrays(esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(10, 10, *want))))
        D = esp.Diagonal(np.random.default_rng(seed).random(10))
        assert isinstance(D * extA, esp.ExtendableSparseMatrix)
        assert isinstance(extA * D, esp.ExtendableSparseMatrix)
