"""GPU: several right-hand sides in one call -- A.mul(X), F.ldiv(V), F.solve(B), A.solve(B) with (n, k) arrays (include/esparse_hip.h,
esp_mul_many / esp_precon_ldiv_many).  The contract is one sentence: column r of the result is, bit for bit, what the
single-vector call gives for column r alone.  For the two panel factorizations (CholeskyFactorization, LUFactorization(form="panels"))
the columns are also held to tests/cholesky_model.c and tests/lu_model.c, so the new kernels are checked against the models and not
only against their single-vector twins.

The new constants T and the sizes that straddle them:
  RC = 8              columns of a chunk (ESP_MANY_CHUNK): the right-hand sides a workgroup of the panel solves carries at once; a
                      narrower last chunk is masked.  Column counts k: 0, 1 (the single-vector path), 2, RC - 1, RC, RC + 1, 2 RC + 1.
  MB = 8              accumulators per lane of the SpMM kernel of A.mul(X) (the same constant): the same k.
  RR = 256 / RC = 32  rows of a node a workgroup walks at once.  Dense nodes n x 1 x 1 with max_depth = 0, n in 1, 2, 31, 32, 33.
  TRI_LDS_MANY = 512  rows of a node's triangle the chunked solves keep in LDS (512 x RC doubles = 32 KiB); a wider node keeps it in
                      the second work vector.  Dense nodes n in 511, 512, 513.
Separators with descendants on both sides: k x k x 1 grids, k in 15, 16, 17, 31, 32, 33.  Struct heights 63 / 64 / 65: the 2-D
grids 61 x 64, 47 x 94, 63 x 66 with leaf_size 4.  The update list of 199 descendants: the arrow's hub.  n = 0."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cholesky_modellib as CM
import lu_modellib as L
from device_views import guarded
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_OK, ESP_ERR_INVALID, ESP_ERR_STATE = 0, -1, -6
RC = 8
TRI = 512
KS = [0, 1, 2, RC - 1, RC, RC + 1, 2 * RC + 1]
KMAX = max(KS)
FORMS = ["cholesky", "lu_columns", "lu_panels"]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    lu = L.Model(tmp_path_factory.mktemp("multi_rhs_lu_model"))
    return {"lu": lu, "cholesky": CM.Model(tmp_path_factory.mktemp("multi_rhs_cholesky_model"), lu=lu)}


def test_constants(esp):
    assert esp._lib.ESP_MANY_CHUNK == RC


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def from_scipy(esp, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    m, n = S.shape
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(m, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def to_device(X):
    """an (n, k) array as a CUDA tensor with stride (1, n)"""
    import torch
    X = np.asarray(X, np.float64)
    return torch.from_numpy(np.ascontiguousarray(X.T).copy()).cuda().t()


def to_host(T):
    return T.cpu().numpy()


def make(esp, form, A, leaf_size=32, max_depth=48):
    if form == "cholesky":
        return esp.CholeskyFactorization(A, leaf_size, max_depth)
    return esp.LUFactorization(A, leaf_size, max_depth, form=form[3:])


_WANT = {}


def model_columns(models, form, key, A, leaf_size, max_depth, V):
    """the model's ldiv of every column of V: computed once per (model, matrix) and shared by the forms (both forms of LU have one
    model), never changed"""
    kind = "cholesky" if form == "cholesky" else "lu"
    if (kind, key) not in _WANT:
        fact = getattr(models[kind], kind)(host_arrays(A), leaf_size, max_depth)
        cols = np.empty(V.shape, order="F")
        for r in range(V.shape[1]):
            cols[:, r] = fact.ldiv(V[:, r])
        cols.setflags(write=False)
        _WANT[(kind, key)] = cols
    return _WANT[(kind, key)]


def rhs(n, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, KMAX)))


def check_factorization(esp, models, form, key, A, leaf_size=32, max_depth=48, lean=False):
    """every k of KS: host arrays (F- and C-ordered), device tensors, in place on both, solve -- against the model's columns and
    against the device's own single-vector ldiv.  lean: every k on host arrays and in place on device tensors, the other ways at
    k = RC + 1 only"""
    n = A.n
    V = rhs(n)
    want = model_columns(models, form, key, A, leaf_size, max_depth, V)
    P = make(esp, form, A, leaf_size, max_depth)
    try:
        stats = (P.stats(), P.panel_stats() if form == "lu_panels" else None)
        single = np.empty((n, KMAX), order="F")
        for r in range(KMAX):
            single[:, r] = P.ldiv(np.ascontiguousarray(V[:, r]))
        assert same_bits(single, want), "the single-vector ldiv against the model"
        for k in KS:
            Vk, Wk = np.asfortranarray(V[:, :k]), want[:, :k]
            U = P.ldiv(Vk)
            assert isinstance(U, np.ndarray) and U.shape == (n, k) and U.flags.f_contiguous and same_bits(U, Wk), (form, k, "host")
            if lean and k != RC + 1:
                T = to_device(Vk)
                assert P.ldiv(T, out=T) is T and same_bits(to_host(T), Wk), (form, k, "device in place")
                continue
            assert same_bits(P.ldiv(np.ascontiguousarray(Vk)), Wk), (form, k, "host, C order")
            assert same_bits(P.solve(Vk), Wk), (form, k, "solve")
            H = Vk.copy(order="F")
            assert P.ldiv(H, out=H) is H and same_bits(H, Wk), (form, k, "host in place")
            T = to_device(Vk)
            D = P.ldiv(T)
            assert D.is_cuda and tuple(D.shape) == (n, k) and same_bits(to_host(D), Wk), (form, k, "device")
            assert same_bits(to_host(T), Vk), (form, k, "the input was written")
            out = P.ldiv(T, out=T)
            assert out is T and same_bits(to_host(T), Wk), (form, k, "device in place")
        assert (P.stats(), P.panel_stats() if form == "lu_panels" else None) == stats     # a many-call changes no counter
    finally:
        P.close()


# ---- the panel factorizations and LU's column form against the models ----------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, TRI - 1, TRI, TRI + 1])
def test_dense_nodes(esp, models, form, n):
    # (the column form of LU takes two launches per column of a dense node and right-hand side: lean where that is a thousand)
    check_factorization(esp, models, form, ("dense", n), esp.fdrand(n, 1, 1), 16, 0, lean=form == "lu_columns" and n > 100)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [15, 16, 17, 31, 32, 33])
def test_separator_widths(esp, models, form, k):
    check_factorization(esp, models, form, ("separator", k), esp.fdrand(k, k, 1))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny", [(61, 64), (47, 94), (63, 66)])
def test_struct_heights(esp, models, form, nx, ny):
    A = from_scipy(esp, L.dominant(L.edges_pattern(nx * ny, L.grid_edges(nx, ny))))
    check_factorization(esp, models, form, ("grid", nx, ny), A, 4)


@pytest.mark.parametrize("form", FORMS)
def test_arrow(esp, models, form):
    check_factorization(esp, models, form, "arrow", from_scipy(esp, L.arrow(200)))


@pytest.mark.parametrize("form", FORMS)
def test_empty_matrix(esp, form):
    P = make(esp, form, esp.ExtendableSparseMatrix(0, 0))
    for k in KS:
        U = P.ldiv(np.empty((0, k), order="F"))
        assert U.shape == (0, k)
        import torch
        D = P.ldiv(torch.empty((k, 0), dtype=torch.float64, device="cuda").t())
        assert tuple(D.shape) == (0, k)
    P.close()


@pytest.mark.parametrize("form", ["columns", "panels"])
def test_backslash(esp, models, form):
    A = esp.fdrand(5, 4, 3)
    B = rhs(A.n)[:, :RC + 1]
    want = model_columns(models, "lu_" + form, "fd60", A, 32, 48, rhs(A.n))[:, :RC + 1]
    X = A.solve(B, form=form)
    assert X.shape == B.shape and X.flags.f_contiguous and same_bits(X, want)
    assert same_bits(esp.solve(A, B, form=form), want)
    assert same_bits(to_host(esp.solve(A, to_device(B), form=form)), want)
    assert same_bits(A.solve(B[:, 0].copy(), form=form), want[:, 0])          # 1-D: as before


# ---- every other kind: the device's own single ldiv, column by column --------------------------------------------------------------------
def interleaved(n):
    return [range(1, n + 1, 2), range(2, n + 1, 2)]


PRECONS = {
    "jacobi": lambda esp, A: esp.JacobiPreconditioner(A),
    "ilu0": lambda esp, A: esp.ILU0Preconditioner(A),
    "iluam": lambda esp, A: esp.ILUAMPreconditioner(A),
    "block": lambda esp, A: esp.BlockPreconditioner(A, interleaved(A.n), esp.ILU0Preconditioner),
    "iluk": lambda esp, A: esp.ILUKPreconditioner(A, 2),
    "ilut": lambda esp, A: esp.ILUTPreconditioner(A),
    "colored": lambda esp, A: esp.ColoredPreconditioner(A),
    "spai0": lambda esp, A: esp.SPAIPreconditioner(A, order=0),
    "spai1": lambda esp, A: esp.SPAIPreconditioner(A, order=1),
    "amg": lambda esp, A: esp.AMGPreconditioner(A, max_coarse=16),
    "rsamg": lambda esp, A: esp.RS_AMGPreconditioner(A, max_coarse=16),
}


@pytest.mark.parametrize("kind", sorted(PRECONS))
def test_other_kinds_column_by_column(esp, kind):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = PRECONS[kind](esp, A)
    try:
        V = rhs(n, seed=5)
        single = np.empty((n, RC + 1), order="F")
        for r in range(RC + 1):
            single[:, r] = P.ldiv(np.ascontiguousarray(V[:, r]))
        for k in (1, 3, RC + 1):
            Vk = np.asfortranarray(V[:, :k])
            assert same_bits(P.ldiv(Vk), single[:, :k]), (kind, k, "host")
            T = to_device(Vk)
            assert same_bits(to_host(P.ldiv(T)), single[:, :k]), (kind, k, "device")
            assert P.ldiv(T, out=T) is T and same_bits(to_host(T), single[:, :k]), (kind, k, "device in place")
    finally:
        P.close()


# ---- A.mul(X) ---------------------------------------------------------------------------------------------------------------------------
def rectangular(esp):
    """257 x 255, row 100 empty"""
    rng = np.random.default_rng(11)
    cnt = 3300
    rows, cols = rng.integers(0, 257, cnt), rng.integers(0, 255, cnt)
    keep = rows != 100
    S = sp.csc_matrix((rng.standard_normal(cnt)[keep], (rows[keep], cols[keep])), shape=(257, 255))
    assert S[100].nnz == 0
    return from_scipy(esp, S)


@pytest.mark.parametrize("name", ["rectangular", "fd60", "empty", "no_columns", "no_rows"])
def test_mul(esp, name):
    A = {"rectangular": lambda: rectangular(esp), "fd60": lambda: esp.fdrand(5, 4, 3), "empty": lambda: esp.ExtendableSparseMatrix(0, 0),
         "no_columns": lambda: esp.ExtendableSparseMatrix(5, 0), "no_rows": lambda: esp.ExtendableSparseMatrix(0, 5)}[name]()
    m, n = A.m, A.n
    X = np.asfortranarray(np.random.default_rng(3).standard_normal((n, KMAX)))
    single = np.empty((m, KMAX), order="F")
    for r in range(KMAX):
        single[:, r] = A.mul(np.ascontiguousarray(X[:, r]))
    if name == "rectangular":
        assert np.all(bits(single[100]) == 0)                                  # the empty row: +0.0
    for k in KS:
        Xk = np.asfortranarray(X[:, :k])
        R = A.mul(Xk)
        assert R.shape == (m, k) and R.flags.f_contiguous and same_bits(R, single[:, :k]), (name, k, "host")
        assert same_bits(A @ np.ascontiguousarray(Xk), single[:, :k]), (name, k, "host, C order, @")
        T = to_device(Xk)
        D = A.mul(T)
        assert tuple(D.shape) == (m, k) and same_bits(to_host(D), single[:, :k]), (name, k, "device")
        out = to_device(np.full((m, k), 7.0))
        assert A.mul(T, out=out) is out and same_bits(to_host(out), single[:, :k]) and same_bits(to_host(T), Xk), (name, k, "device, out")


# ---- independence of the columns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS + ["ilu0", "amg"])
def test_nan_and_inf_stay_in_their_columns(esp, form):
    A = esp.fdrand(9, 9, 1)
    n = A.n
    P = PRECONS[form](esp, A) if form in PRECONS else make(esp, form, A, 8)
    try:
        V = rhs(n, seed=9)[:, :RC + 2]
        clean = P.ldiv(V)
        assert np.all(np.isfinite(clean))
        W = V.copy(order="F")
        W[n // 2, 1] = np.nan
        W[n // 3, 2] = np.inf
        for got in (P.ldiv(W), to_host(P.ldiv(to_device(W)))):
            others = [r for r in range(W.shape[1]) if r not in (1, 2)]
            assert same_bits(got[:, others], clean[:, others])
            assert not np.all(np.isfinite(got[:, 1])) and not np.all(np.isfinite(got[:, 2]))
            for r in (1, 2):
                assert same_bits(got[:, r], P.ldiv(np.ascontiguousarray(W[:, r])))
    finally:
        P.close()


@pytest.mark.parametrize("form", FORMS + ["jacobi"])
def test_negative_zero_survives_where_the_single_call_keeps_it(esp, form):
    A = esp.fdrand(6, 5, 1)
    n = A.n
    P = PRECONS[form](esp, A) if form in PRECONS else make(esp, form, A, 8)
    try:
        V = np.zeros((n, RC + 1), order="F")
        V[:, 1] = -0.0
        V[:, RC] = -0.0
        V[0, 2] = 1.0
        single = np.stack([P.ldiv(np.ascontiguousarray(V[:, r])) for r in range(V.shape[1])], axis=1)
        got = P.ldiv(V)
        assert np.array_equal(bits(got), bits(single))                         # the sign bits included
        assert np.array_equal(bits(to_host(P.ldiv(to_device(V)))), bits(single))
        X = np.zeros((n, 3), order="F")
        X[:, 1] = -0.0
        assert np.array_equal(bits(A.mul(X)), bits(np.stack([A.mul(np.ascontiguousarray(X[:, r])) for r in range(3)], axis=1)))
    finally:
        P.close()


# ---- leading dimensions and guard bands ------------------------------------------------------------------------------------------------------
PAD_BITS = 0x7FF8DEADBEEF5A5B    # device_views' float64 canary


def strided(esp, values, ld, lead, device):
    """(view, whole, check): the (n, k) `values` as a column-major view with leading dimension ld at element offset `lead` of a
    guarded buffer; the ld - n pad rows between the columns hold the canary NaN and belong to `whole` (ld * k elements)"""
    import torch
    n, k = values.shape
    flat = np.empty(ld * k)
    flat.view(np.uint64)[:] = PAD_BITS
    for r in range(k):
        flat[r * ld:r * ld + n] = values[:, r]
    g = guarded(torch.from_numpy(flat).cuda() if device else flat, lead)
    if device:
        view = torch.as_strided(g.view, (n, k), (1, ld))
    else:
        view = np.lib.stride_tricks.as_strided(g.view, (n, k), (8, 8 * ld))
    return view, g.view, g.check


def pads_intact(whole, n, ld, k):
    w = whole.cpu().numpy() if hasattr(whole, "cpu") else whole
    w = w.view(np.uint64).reshape(k, ld)
    return bool(np.all(w[:, n:] == PAD_BITS))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("form", FORMS + ["ilu0"])
def test_leading_dimensions_and_guard_bands(esp, form, device):
    A = esp.fdrand(7, 6, 1)
    n = A.n
    ld, k = n + 3, RC + 1
    P = PRECONS[form](esp, A) if form in PRECONS else make(esp, form, A, 8)
    try:
        V = rhs(n, seed=4)[:, :k]
        want = P.ldiv(V)
        v, vwhole, vcheck = strided(esp, V, ld, 1, device)
        u, uwhole, ucheck = strided(esp, np.full((n, k), 7.0), ld, 3, device)
        got = P.ldiv(v, out=u)
        A.synchronize()
        assert got is u
        got = to_host(got) if device else got
        assert not np.any(np.isnan(got)) and same_bits(got, want)              # the NaN pad rows of V were never read
        assert same_bits(to_host(v) if device else v, V) and pads_intact(vwhole, n, ld, k)
        assert pads_intact(uwhole, n, ld, k)                                   # the pad rows of U were never written
        vcheck("V"), ucheck("U")
        assert P.ldiv(v, out=v) is v                                           # in place behind the same guards
        A.synchronize()
        assert same_bits(to_host(v) if device else v, want) and pads_intact(vwhole, n, ld, k)
        vcheck("V = U")
    finally:
        P.close()


@pytest.mark.parametrize("device", [False, True])
def test_mul_leading_dimensions_and_guard_bands(esp, device):
    A = rectangular(esp)
    m, n, k = A.m, A.n, RC + 1
    X = np.asfortranarray(np.random.default_rng(2).standard_normal((n, k)))
    want = A.mul(X)
    x, xwhole, xcheck = strided(esp, X, n + 3, 1, device)
    r, rwhole, rcheck = strided(esp, np.full((m, k), 7.0), m + 5, 3, device)
    got = A.mul(x, out=r)
    A.synchronize()
    assert got is r
    got = to_host(got) if device else got
    assert not np.any(np.isnan(got)) and same_bits(got, want)
    assert pads_intact(xwhole, n, n + 3, k) and pads_intact(rwhole, m, m + 5, k)
    xcheck("X"), rcheck("R")


# ---- error codes ---------------------------------------------------------------------------------------------------------------------------
def dev_ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 8 * offset)


@pytest.mark.parametrize("form", ["cholesky", "lu_panels", "ilu0"])
def test_ldiv_many_error_codes(esp, form):
    import torch
    A = esp.fdrand(5, 4, 3)
    n = A.n
    lib = A._d.lib
    P = PRECONS[form](esp, A) if form in PRECONS else make(esp, form, A, 8)
    try:
        p = P._live()
        buf = torch.zeros((RC + 2) * n, dtype=torch.float64, device="cuda")
        other = torch.zeros((RC + 2) * n, dtype=torch.float64, device="cuda")
        call = lambda V, ldv, U, ldu, k: lib.esp_precon_ldiv_many(p, V, ldv, U, ldu, k, 1)
        assert call(dev_ptr(buf), n, dev_ptr(other), n, 0) == ESP_OK
        assert call(None, n, None, n, 0) == ESP_OK                               # nothing to read or write
        assert call(dev_ptr(buf), n, dev_ptr(other), n, -1) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), n - 1, dev_ptr(other), n, 2) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), n, dev_ptr(other), n - 1, 2) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), 0, dev_ptr(other), n, 0) == ESP_ERR_INVALID     # ld < max(n, 1) whatever k is
        assert call(None, n, dev_ptr(other), n, 2) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), n, None, n, 2) == ESP_ERR_INVALID
        # overlaps: U inside V's range, shifted by a column, by one element, and U == V with another leading dimension
        assert call(dev_ptr(buf), n, dev_ptr(buf, n), n, 3) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), n, dev_ptr(buf, 1), n, 3) == ESP_ERR_INVALID
        assert call(dev_ptr(buf, 3 * n - 1), n, dev_ptr(buf), n, 3) == ESP_ERR_INVALID
        assert call(dev_ptr(buf), n, dev_ptr(buf), n + 1, 3) == ESP_ERR_INVALID
        assert not bool(buf.any()) and not bool(other.any())                     # refused before anything was launched
        assert call(dev_ptr(buf), n, dev_ptr(buf, 3 * n), n, 3) == ESP_OK        # touching ranges do not overlap
        assert call(dev_ptr(buf), n, dev_ptr(buf), n, 3) == ESP_OK               # in place
        assert lib.esp_precon_ldiv_many(None, dev_ptr(buf), n, dev_ptr(other), n, 1, 1) == ESP_ERR_INVALID
        A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.25, 0.25])                   # a pattern change without update()
        A.flush()
        for k in (0, 1, 2, RC + 1):
            assert call(dev_ptr(buf), n, dev_ptr(other), n, k) == ESP_ERR_STATE
        with pytest.raises(esp.EspError) as e:
            P.ldiv(np.zeros((n, 2), order="F"))
        assert e.value.code == ESP_ERR_STATE
    finally:
        P.close()


def test_mul_many_error_codes(esp):
    import torch
    A = rectangular(esp)
    m, n = A.m, A.n
    lib, h = A._d.lib, A._d.h
    x = torch.zeros(4 * m, dtype=torch.float64, device="cuda")
    r = torch.zeros(4 * m, dtype=torch.float64, device="cuda")
    call = lambda X, ldx, R, ldr, k: lib.esp_mul_many(h, X, ldx, R, ldr, k, 1)
    assert call(dev_ptr(x), n, dev_ptr(r), m, 0) == ESP_OK
    assert call(dev_ptr(x), n, dev_ptr(r), m, 3) == ESP_OK
    assert call(dev_ptr(x), n, dev_ptr(r), m, -1) == ESP_ERR_INVALID
    assert call(dev_ptr(x), n - 1, dev_ptr(r), m, 2) == ESP_ERR_INVALID
    assert call(dev_ptr(x), n, dev_ptr(r), m - 1, 2) == ESP_ERR_INVALID
    assert call(None, n, dev_ptr(r), m, 2) == ESP_ERR_INVALID
    assert call(dev_ptr(x), n, None, m, 2) == ESP_ERR_INVALID
    assert call(dev_ptr(x), n, dev_ptr(x), m, 2) == ESP_ERR_INVALID             # X and R overlap
    assert call(dev_ptr(x), n, dev_ptr(x, 2 * n - 1), m, 2) == ESP_ERR_INVALID
    assert lib.esp_mul_many(None, dev_ptr(x), n, dev_ptr(r), m, 1, 1) == ESP_ERR_INVALID
    A.append(esp.ESP_UPDATE, [1], [1], [1.0])                                   # pending entries
    for k in (0, 1, 2):
        assert call(dev_ptr(x), n, dev_ptr(r), m, k) == ESP_ERR_STATE
    A.flush()
    assert call(dev_ptr(x), n, dev_ptr(r), m, 2) == ESP_OK


def test_python_refusals(esp):
    import torch
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.CholeskyFactorization(A, 8)
    try:
        bad = [np.zeros((n + 1, 2)), np.zeros((n, 2, 2)), np.zeros((n, 2), np.float32),
               torch.zeros((n, 2), dtype=torch.float64, device="cuda"),                    # row-major: stride(0) != 1
               torch.zeros((2, n), dtype=torch.float32, device="cuda").t(),
               torch.zeros((2, n + 1), dtype=torch.float64, device="cuda").t()]
        for X in bad:
            with pytest.raises(ValueError, match="DimensionMismatch"):
                P.ldiv(X)
            with pytest.raises(ValueError, match="DimensionMismatch"):
                A.mul(X)
        with pytest.raises(ValueError, match="DimensionMismatch"):
            P.ldiv(np.zeros((n, 2), order="F"), out=np.zeros((n, 3), order="F"))
        with pytest.raises(ValueError):
            P.ldiv(np.zeros((n, 2), order="F"), out=np.zeros((n, 2)))                      # a C-ordered out cannot be written in place
    finally:
        P.close()


# ---- updates ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_values_only_update_is_followed(esp, models, form):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = make(esp, form, A, 8)
    try:
        V = rhs(n, seed=6)[:, :RC + 1]
        old = P.ldiv(V)
        csc = A.sparse()
        csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
        A._push_edits()
        assert same_bits(P.ldiv(V), old)                          # no update(): the factorization holds copies
        P.update()
        kind = "cholesky" if form == "cholesky" else "lu"
        fact = getattr(models[kind], kind)(host_arrays(A), 8)
        new = np.stack([fact.ldiv(V[:, r]) for r in range(V.shape[1])], axis=1)
        assert same_bits(P.ldiv(V), new) and same_bits(to_host(P.ldiv(to_device(V))), new) and not same_bits(new, old)
    finally:
        P.close()
