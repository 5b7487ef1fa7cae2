"""GPU: transpose, transpose(A)*x, issymmetric, opnorm and norm on the device CSC (include/esparse_hip.h: esp_transpose,
esp_mul_transpose, esp_issymmetric, esp_opnorm, esp_norm) against the independent model of tests/linalg_model.c -- bitwise
where SparseArrays is exact, within 1e-13 of an exactly rounded reference where it calls BLAS."""
import ctypes
import math

import numpy as np
import pytest

from linalg_modellib import Model, norm_exact, norm_ref
from refmodel import bits
from test_matops_gpu import arrays, canon, ext, rand_csc

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6
INF = math.inf


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("linalg_model"))


def assert_raw(got, want, what=""):
    """colptr, rowval and the RAW bits of nzval (no NaN canonicalisation: a transpose moves data only)"""
    (cp1, rv1, nz1), (cp2, rv2, nz2) = got, want
    assert np.array_equal(cp1, cp2), what + " colptr differs"
    assert np.array_equal(rv1, rv2), what + " rowval differs"
    assert np.array_equal(bits(nz1), bits(nz2)), what + " nzval differs (raw bits)"


def check_transpose(esp, model, A):
    want = model.transpose(A.m, arrays(A))
    got = []
    for path in (1, 2, 0):
        T = A.transpose(path=path)
        assert isinstance(T, esp.ExtendableSparseMatrix) and T.shape == (A.n, A.m) and T.nnznew() == 0
        g = arrays(T)
        assert_raw(g, want, "transpose path %d" % path)
        got.append(g)
    assert_raw(got[0], got[1], "generic vs counting")
    return want


def nonsymmetric(esp):
    from test_precon_gpu import nonsymmetric as ns
    return ns(esp)


def from_values(esp, m, n, density, seed, vals):
    return ext(esp, m, rand_csc(m, n, density, seed, vals))


# ---- transpose ------------------------------------------------------------------------------------------------------------
def test_transpose_fdrand40(esp, model):
    A = esp.fdrand(40, 40, 40, rand_mode=1, seed=21)
    check_transpose(esp, model, A)
    assert_raw(arrays(A.transpose()), arrays(A), "fdrand is symmetric")


def test_transpose_nonsymmetric(esp, model):
    A = nonsymmetric(esp)
    want = check_transpose(esp, model, A)
    assert not np.array_equal(want[1], arrays(A)[1])


@pytest.mark.parametrize("m,n,d", [(300, 200, 0.02), (1, 500, 0.5), (700, 1, 0.5), (1, 3000, 1.0), (1, 6000, 1.0),
                                   (200, 5000, 0.3)])
def test_transpose_rectangular(esp, model, m, n, d):
    """1 x n and n x 1, a row of 3000 entries (the workgroup sort) and of 6000 (path 2 hands it to the generic path), rows of
    ~1500 entries (many workgroup sorts)"""
    check_transpose(esp, model, ext(esp, m, rand_csc(m, n, d, 1)))


def test_transpose_row_lengths_of_every_tier(esp, model):
    """C columns of 1..40 entries and a few long ones: every lane-sort width (8, 16, 32) and the workgroup sort"""
    for top in (5, 12, 30, 40, 300):
        rng = np.random.default_rng(top)
        m, n = 400, 600
        lens = rng.integers(0, top + 1, m)
        I = np.repeat(np.arange(1, m + 1), lens)
        J = np.concatenate([np.sort(rng.choice(n, L, replace=False)) + 1 for L in lens]) if lens.sum() else np.zeros(0, np.int64)
        A = esp.ExtendableSparseMatrix(m, n)
        A.append(esp.ESP_UPDATE, I, J, rng.standard_normal(len(I)))
        A.flush()
        check_transpose(esp, model, A)


def test_transpose_empty_and_zero_values(esp, model):
    Z = esp.ExtendableSparseMatrix(30, 20)
    for path in (1, 2):
        T = Z.transpose(path=path)
        cp, rv, nz = arrays(T)
        assert T.shape == (20, 30) and len(rv) == 0 and np.all(cp == 1) and len(cp) == 31
    zeros = lambda k: np.resize(np.array([0.0, -0.0]), k)
    A = from_values(esp, 120, 90, 0.05, 2, zeros)
    want = check_transpose(esp, model, A)
    assert len(want[1]) == A.nnz() > 0


def test_transpose_negative_zero_and_nan_payloads(esp, model):
    pay = np.array([0x7FF800000000BEEF, 0xFFF8000000001234, 0x8000000000000000, 0x7FF0000000000000, 0x0000000000000001],
                   np.uint64).view(np.float64)
    vals = lambda k: np.resize(np.concatenate([pay, [1.5, -2.0, 0.0]]), k)
    A = from_values(esp, 150, 170, 0.06, 3, vals)
    want = check_transpose(esp, model, A)
    for b in bits(pay):
        assert np.any(bits(want[2]) == b)


def test_transpose_twice_and_live_result(esp, orc, model):
    A = ext(esp, 200, rand_csc(200, 150, 0.03, 4))
    for path in (1, 2):
        TT = A.transpose(path=path).transpose(path=path)
        assert_raw(arrays(TT), arrays(A), "transpose(transpose(A))")
    T = A.transpose()
    cp, rv, nz = arrays(T)
    O = orc.ExtendableSparseMatrix(orc.CSC(150, 200, cp, rv, nz))
    rng = np.random.default_rng(5)
    J = np.repeat(np.arange(1, 201), np.diff(cp))
    stored = rng.integers(0, len(rv), 200)
    I = np.concatenate([rv[stored], rng.integers(1, 151, 200)])
    Jc = np.concatenate([J[stored], rng.integers(1, 201, 200)])
    V = rng.standard_normal(400)
    for i, j, v in zip(I, Jc, V):
        T.updateindex("+", v, int(i), int(j))
        O.updateindex(orc.OP_ADD, v, int(i), int(j))
    T.flush()
    O.flush()
    assert_raw(arrays(T), O.arrays(), "T after updates")
    assert T.phash == esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(150, 200, *arrays(T))).phash


# ---- transpose(A)*x -------------------------------------------------------------------------------------------------------
def check_mul_transpose(esp, model, A, x):
    want = model.mul_transpose(arrays(A), x)
    got = A.mul_transpose(x)
    assert got.shape == (A.n,)
    assert np.array_equal(canon(got), canon(want))
    import torch
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    gt = A.mul_transpose(xt).cpu().numpy()
    assert np.array_equal(canon(gt), canon(want))
    return want


def test_mul_transpose_rectangular_and_long_columns(esp, model):
    rng = np.random.default_rng(6)
    A = ext(esp, 300, rand_csc(300, 200, 0.05, 7))
    check_mul_transpose(esp, model, A, rng.standard_normal(300))
    # dense columns (thousands of entries: the wave path) next to short ones
    L = ext(esp, 5000, rand_csc(5000, 70, 0.3, 8))
    check_mul_transpose(esp, model, L, rng.standard_normal(5000))
    check_mul_transpose(esp, model, nonsymmetric(esp), rng.standard_normal(3000))


def test_mul_transpose_inf_nan(esp, model):
    rng = np.random.default_rng(9)
    A = ext(esp, 400, rand_csc(400, 300, 0.05, 10))
    x = rng.standard_normal(400)
    x[::17] = INF
    x[5::23] = -INF
    x[7::31] = np.nan
    want = check_mul_transpose(esp, model, A, x)
    assert np.isnan(want).any() and np.isinf(want).any()
    L = ext(esp, 3000, rand_csc(3000, 8, 0.5, 11))
    check_mul_transpose(esp, model, L, np.resize(x, 3000))


# ---- issymmetric ----------------------------------------------------------------------------------------------------------
def csc_of(esp, m, n, I, J, V):
    """a CSC with exactly these entries (no folding: positions distinct), stored zeros kept"""
    order = np.lexsort((I, J))
    I, J, V = np.asarray(I)[order], np.asarray(J)[order], np.asarray(V, np.float64)[order]
    cp = np.concatenate([[1], 1 + np.cumsum(np.bincount(np.asarray(J) - 1, minlength=n))]).astype(np.int64)
    return ext(esp, m, (cp, np.asarray(I, np.int64), V))


def test_issymmetric_small_cases(esp, model):
    def sym(A):
        got = A.issymmetric()
        assert A.ishermitian() == got
        if A.m * A.n <= 10 ** 7:  # (the model builds the dense matrix)
            assert got == model.issymmetric(A.m, arrays(A))
        return got
    base_I, base_J, base_V = [1, 2, 1, 3, 2, 3], [1, 1, 2, 2, 3, 3], [4.0, 1.5, 1.5, 2.0, 2.0, 5.0]
    assert sym(csc_of(esp, 3, 3, base_I, base_J, base_V))
    assert not sym(csc_of(esp, 3, 3, base_I, base_J, [4.0, 1.5, 1.25, 2.0, 2.0, 5.0]))    # one off-diagonal differs
    assert sym(csc_of(esp, 3, 3, base_I + [3], base_J + [1], base_V + [0.0]))             # stored zero, no mirror
    assert sym(csc_of(esp, 3, 3, base_I + [3], base_J + [1], base_V + [-0.0]))
    assert sym(csc_of(esp, 3, 3, base_I + [3, 1], base_J + [1, 3], base_V + [0.0, -0.0]))  # +0.0 against -0.0
    assert not sym(csc_of(esp, 3, 3, base_I, base_J, [np.nan, 1.5, 1.5, 2.0, 2.0, 5.0]))  # NaN on the diagonal
    assert not sym(csc_of(esp, 3, 3, base_I, base_J, [4.0, np.nan, np.nan, 2.0, 2.0, 5.0]))
    assert not sym(csc_of(esp, 3, 3, base_I + [3], base_J + [1], base_V + [1.0]))          # no mirror
    assert not sym(ext(esp, 30, rand_csc(30, 20, 0.3, 12)))                                # rectangular
    assert sym(esp.ExtendableSparseMatrix(7, 7)) and not sym(esp.ExtendableSparseMatrix(7, 6))
    assert sym(esp.fdrand(20, 20, 20, rand_mode=1, seed=13))
    assert not sym(nonsymmetric(esp))


# ---- opnorm and norm ------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or bits(np.array([a]))[0] == bits(np.array([b]))[0]


def close(got, want):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want) or want == 0.0:
        return got == want
    return abs(got - want) <= 1e-13 * abs(want)


NORM_P = (INF, -INF, 0, 1, 2, 3, 0.5, -2.5)


def check_norms(A, nz):
    for p in NORM_P:
        g = A.norm(p)
        assert same_bits(g, A.norm(p)), ("norm not reproducible", p)
        e = norm_exact(nz, p)
        if e is not None:
            assert same_bits(g, e), ("norm", p, g, e)
        else:
            assert close(g, norm_ref(nz, p)), ("norm", p, g, norm_ref(nz, p))


def test_opnorm_general_branch(esp, model):
    vals = lambda k: np.resize(np.array([0.0, -0.0, 1.5, -2.0, 3.25, -7.0, 0.1]), k)
    for m, n, seed in ((300, 200, 14), (2, 500, 15), (500, 2, 16)):
        A = from_values(esp, m, n, 0.05, seed, vals)
        a = arrays(A)
        for p in (1, INF):
            assert same_bits(A.opnorm(p), model.opnorm_general(m, a, p)), (m, n, p)
        check_norms(A, a[2])
    A = nonsymmetric(esp)
    for p in (1, INF):
        assert same_bits(A.opnorm(p), model.opnorm_general(A.m, arrays(A), p))


def test_opnorm_nan_inf(esp, model):
    for special in (np.nan, INF, -INF):
        vals = lambda k: np.resize(np.array([1.0, -2.0, special, 0.5]), k)
        A = from_values(esp, 80, 60, 0.1, 17, vals)
        a = arrays(A)
        for p in (1, INF):
            g, w = A.opnorm(p), model.opnorm_general(80, a, p)
            assert same_bits(g, w) and (math.isnan(g) if np.isnan(special) else g == INF)
        check_norms(A, a[2])


def test_opnorm_one_row_and_one_column(esp):
    rng = np.random.default_rng(18)
    for m, n in ((1, 700), (700, 1), (1, 1)):
        A = ext(esp, m, rand_csc(m, n, 0.6, 19, lambda k: rng.standard_normal(k)))
        nz = arrays(A)[2]
        if m == 1:
            assert same_bits(A.opnorm(1), norm_exact(nz, INF))
            assert close(A.opnorm(2), norm_ref(nz, 2)) and close(A.opnorm(INF), norm_ref(nz, 1))
        else:
            assert same_bits(A.opnorm(INF), norm_exact(nz, INF))
            assert close(A.opnorm(2), norm_ref(nz, 2)) and close(A.opnorm(1), norm_ref(nz, 1))
        assert same_bits(A.opnorm(2), A.opnorm(2))
        with pytest.raises(ValueError):
            A.opnorm(3)
    R = ext(esp, 1, (np.array([1, 1, 1, 1]), np.zeros(0, np.int64), np.zeros(0)))  # 1 x 3, nothing stored
    assert R.opnorm(1) == 0.0 and R.opnorm(2) == 0.0 and R.opnorm(INF) == 0.0


def test_opnorm_empty_and_refusals(esp):
    lib = esp._lib.load()
    for m, n in ((0, 5), (5, 0), (0, 0)):
        E = esp.ExtendableSparseMatrix(m, n)
        assert E.opnorm(1) == 0.0 and E.opnorm(2) == 0.0 and E.opnorm(3) == 0.0
    A = ext(esp, 30, rand_csc(30, 20, 0.2, 20))
    with pytest.raises(ValueError, match="2-norm not yet implemented"):
        A.opnorm(2)
    with pytest.raises(ValueError, match="invalid operator norm"):
        A.opnorm(3)
    with pytest.raises(ValueError):
        A.opnorm(math.nan)
    with pytest.raises(ValueError):
        A.norm(math.nan)
    r = ctypes.c_double()
    assert lib.esp_opnorm(A._d.h, 2.0, ctypes.byref(r)) == ESP_ERR_UNSUPPORTED
    assert lib.esp_opnorm(A._d.h, 0.5, ctypes.byref(r)) == ESP_ERR_INVALID
    assert lib.esp_opnorm(A._d.h, math.nan, ctypes.byref(r)) == ESP_ERR_INVALID
    assert lib.esp_norm(A._d.h, math.nan, ctypes.byref(r)) == ESP_ERR_INVALID
    Z = esp.ExtendableSparseMatrix(9, 9)
    for p in NORM_P:
        assert Z.norm(p) == 0.0
    assert Z.opnorm(1) == 0.0 and Z.opnorm(INF) == 0.0


def test_norm_extreme_magnitudes(esp):
    rng = np.random.default_rng(21)
    for scale in (1e200, 1e-200, 1.0):
        A = ext(esp, 400, rand_csc(400, 300, 0.05, 22, lambda k: scale * rng.standard_normal(k)))
        nz = arrays(A)[2]
        g = A.norm(2)
        assert math.isfinite(g) and g > 0 and close(g, norm_ref(nz, 2))
        check_norms(A, nz)
    Z = from_values(esp, 50, 50, 0.1, 23, lambda k: np.resize(np.array([0.0, -0.0]), k))
    check_norms(Z, arrays(Z)[2])


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(esp):
    lib = esp._lib.load()
    z, r, f = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int32()
    A = ext(esp, 30, rand_csc(30, 20, 0.2, 30))
    x = np.ones(30)
    y = np.empty(20)
    A.updateindex("+", 1.0, 1, 1)
    A._d.commit()
    h = A._d.h
    assert lib.esp_transpose(h, esp.ExtendableSparseMatrix(20, 30)._d.h, ctypes.byref(z)) == ESP_ERR_STATE
    assert lib.esp_mul_transpose(h, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 0) == ESP_ERR_STATE
    assert lib.esp_issymmetric(h, ctypes.byref(f)) == ESP_ERR_STATE
    assert lib.esp_opnorm(h, 1.0, ctypes.byref(r)) == ESP_ERR_STATE
    assert lib.esp_norm(h, 2.0, ctypes.byref(r)) == ESP_ERR_STATE
    A.flush()
    assert lib.esp_transpose(h, h, ctypes.byref(z)) == ESP_ERR_INVALID
    assert lib.esp_transpose(h, esp.ExtendableSparseMatrix(30, 20)._d.h, ctypes.byref(z)) == ESP_ERR_INVALID
    assert lib.esp_debug_transpose_path(h, 3) == ESP_ERR_INVALID
    with pytest.raises(ValueError, match="DimensionMismatch"):
        A.mul_transpose(np.ones(20))
    # a column window
    W = esp.ExtendableSparseMatrix(40, 40)
    W.set_column_window(1, 10)
    W.append(esp.ESP_UPDATE, np.arange(1, 11), np.arange(1, 11), np.ones(10))
    W.flush()
    assert lib.esp_transpose(W._d.h, esp.ExtendableSparseMatrix(40, 40)._d.h, ctypes.byref(z)) == ESP_ERR_UNSUPPORTED
    assert lib.esp_norm(W._d.h, 2.0, ctypes.byref(r)) == ESP_ERR_UNSUPPORTED


def test_failed_transpose_leaves_the_result_intact(esp, model):
    A = esp.fdrand(30, 30, 30, rand_mode=1, seed=31)
    prev = rand_csc(27000, 27000, 0.0005, 32)
    C = ext(esp, 27000, prev)
    lib = esp._lib.load()
    lib.esp_debug_fail_next_bucket_stage(C._d.h)
    assert lib.esp_debug_transpose_path(C._d.h, 1) == 0
    z = ctypes.c_int64()
    assert lib.esp_transpose(A._d.h, C._d.h, ctypes.byref(z)) == ESP_ERR_STATE
    C._host_state = C.HOST_STALE  # (read the device CSC, not the host copy made at upload)
    assert_raw(arrays(C), prev, "c after a failed transpose")
    assert C.nnznew() == 0
    # the next call goes through and replaces c's CSC
    assert lib.esp_transpose(A._d.h, C._d.h, ctypes.byref(z)) == 0 and z.value == A.nnz()
    C._host_state = C.HOST_STALE
    assert_raw(arrays(C), model.transpose(A.m, arrays(A)), "c after the next transpose")


# ---- 256^3 ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(esp):
    A = esp.fdrand(256, 256, 256, rand_mode=1, seed=0x5EED0002)
    return A, arrays(A)


def test_transpose_256(esp, big):
    A, a = big
    for path in (1, 2):
        T = A.transpose(path=path)
        assert_raw(arrays(T), a, "transpose(fdrand 256^3), path %d" % path)
        del T
    d = np.random.default_rng(40).standard_normal(A.n)
    D = esp.Diagonal(d)
    AD = A * D
    T = AD.transpose()
    del AD
    DA = D * A
    assert_raw(arrays(T), arrays(DA), "transpose(A*D) == D*A")


def test_linalg_256(esp, model, big):
    A, (cp, rv, nz) = big
    x = np.random.default_rng(41).standard_normal(A.n)
    r1 = A.mul(x)
    r2 = A.mul_transpose(x)
    assert np.array_equal(bits(r1), bits(r2)), "transpose(A)*x == A*x on the symmetric fdrand"
    assert A.issymmetric()
    for p in (1, INF):
        assert same_bits(A.opnorm(p), model.opnorm_general(A.m, (cp, rv, nz), p)), p
    for p in (INF, -INF, 0):
        assert same_bits(A.norm(p), norm_exact(nz, p)), p
    a = np.abs(nz)
    s = float(a.max())
    CH = 1 << 23
    sq = sum(np.sum((np.asarray(a[i:i + CH], np.longdouble) / s) ** 2) for i in range(0, len(a), CH))
    ab = sum(np.sum(np.asarray(a[i:i + CH], np.longdouble)) for i in range(0, len(a), CH))
    sq, ab = float(sq), float(ab)
    for p, want in ((2, s * math.sqrt(sq)), (1, ab)):
        g = A.norm(p)
        assert same_bits(g, A.norm(p)) and abs(g - want) <= 1e-13 * want, (p, g, want)
    # one perturbed off-diagonal value
    i, j = int(rv[cp[100] - 1]), 101
    assert i != j
    A[i, j] = A[i, j] + 1.0
    assert not A.issymmetric()
