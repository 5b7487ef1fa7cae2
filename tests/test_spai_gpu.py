"""GPU: SPAIPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_spai_create) against tests/spai_model.c: M's
colptr, rowval and value bits (a NaN equal to a NaN in the same position), the sizes of the local problems, both tiers, the
refusal of a too-large column, update!, ldiv! and the solvers' whole histories, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_modellib
from bicgstabl_modellib import convdiff_triplets
from refmodel import bits
from spai_modellib import Model, SolverModel, csc_from_columns, hub_columns, sized_columns, too_large_columns

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("spai_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("spai_gmres_model"))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def from_arrays(esp, csc):
    cp, rv, nz = csc
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(len(cp) - 1, len(cp) - 1, cp, rv, nz))


def from_scipy(esp, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return from_arrays(esp, (S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)))


def convdiff(esp, nx, ny, nz, pe):
    I, J, V = convdiff_triplets(nx, ny, nz, pe)
    A = esp.ExtendableSparseMatrix(nx * ny * nz, nx * ny * nz)
    A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def check_matrix(P, want):
    cp, rv, nz = P.matrix()
    assert np.array_equal(cp, want.M[0]) and np.array_equal(rv, want.M[1])
    assert same_bits(nz, want.M[2]) and same_bits(P.factor(), want.M[2])
    st = P.stats()
    assert (st["max_p"], st["max_q"], st["max_pq"]) == want.stats
    assert P.levels_launches() == ((0, 0, 0), (0,) * 6)


def check_ldiv(P, want, seed=1):
    import torch
    n = want.n
    v = np.random.default_rng(seed).standard_normal(n)
    with np.errstate(all="ignore"):
        u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u)
    if n == 0:                                           # (a device vector without elements has no address)
        return u
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)                               # u aliases v, device pointers
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    t2 = torch.empty_like(t)
    P.ldiv(torch.from_numpy(v.copy()).cuda(), out=t2)    # device pointers, u apart from v
    assert same_bits(t2.cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


class Spai:
    """SPAIPreconditioner with the two read-only calls every kind answers (zeros here)"""

    def __init__(self, esp, A, order=1, symmetric=False):
        self.P = esp.SPAIPreconditioner(A, order, symmetric)
        self.A = A

    def __getattr__(self, name):
        return getattr(self.P, name)

    def levels_launches(self):
        lib, p = self.A._d.lib, self.P._live()
        lev, lau = (C.c_int64 * 3)(), (C.c_int64 * 6)()
        assert lib.esp_precon_levels(p, lev) == 0 and lib.esp_precon_launches(p, lau) == 0
        return tuple(lev), tuple(lau)


def check_all(esp, model, A, symmetric=False, arrays=None):
    arrays = host_arrays(A) if arrays is None else arrays
    with np.errstate(all="ignore"):
        want = model.precon(arrays, 1, symmetric)
    P = Spai(esp, A, 1, symmetric)
    try:
        check_matrix(P, want)
        check_ldiv(P, want)
        return P.stats(), want
    finally:
        P.close()


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def shape(esp, name):
    if name == "n0":
        A = esp.ExtendableSparseMatrix(0, 0)
        A.flush()
        return A
    if name == "n1":
        return from_scipy(esp, sp.csc_matrix(np.array([[4.0]])))
    if name == "diag":
        return from_scipy(esp, sp.diags([np.arange(2.0, 9.0)], [0]))
    if name == "tri5":
        return from_scipy(esp, sp.diags([[-1.0, -2.0, -1.5, -0.5], [4.0, 5.0, 6.0, 7.0, 8.0], [-2.0, -1.0, -3.0, -0.25]], [-1, 0, 1]))
    if name == "cd4":
        return convdiff(esp, 4, 4, 4, 4.0)
    assert name == "fd5x4x3"
    return esp.fdrand(5, 4, 3)


@pytest.mark.parametrize("name", ["n0", "n1", "diag", "tri5", "fd5x4x3", "cd4"])
@pytest.mark.parametrize("symmetric", [False, True])
def test_shapes(esp, model, name, symmetric):
    A = shape(esp, name)
    st, want = check_all(esp, model, A, symmetric)
    assert st["wide"] == 0
    if name == "diag":
        assert np.array_equal(want.M[2], 1.0 / np.arange(2.0, 9.0))
    if symmetric:
        P = esp.SPAIPreconditioner(A, 1, True)
        assert P.issymmetric()
        P.close()


@pytest.mark.parametrize("name", ["n0", "n1", "tri5", "fd5x4x3", "cd4"])
def test_order0(esp, model, name):
    A = shape(esp, name)
    want = model.precon(host_arrays(A), 0)
    P = esp.SPAIPreconditioner(A, 0)
    assert same_bits(P.factor(), want.diag)
    check_ldiv(P, want)
    assert P.stats() == {"max_p": 0, "max_q": 0, "max_pq": 0, "wide": 0}
    with pytest.raises(esp.EspError) as e:
        P.matrix()
    assert e.value.code == ESP_ERR_INVALID
    P.close()
    Q = esp.AMGCL_RLXPreconditioner(A, type="spai0")
    assert Q.order == 0 and same_bits(Q.factor(), want.diag)
    Q.close()


# ---- the ordered sum's strides and the tiers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [63, 64, 65, 130])
def test_hub_columns(esp, model, h):
    """column 1 has p = h + 1 rows: one, two and three lane strides of the ordered sum; the hub itself is the workgroup tier's
    (q = h unknowns over 3 rows: p < q, rank-deficient -- the NaN pattern is the model's)"""
    csc = csc_from_columns(hub_columns(h), np.random.default_rng(h))
    st, want = check_all(esp, model, from_arrays(esp, csc), arrays=csc)
    assert st["max_p"] == h + 1 and st["max_q"] == h and st["wide"] == 1
    assert want.pcol[1] == h + 1 and np.all(np.isfinite(want.M[2][csc[0][1] - 1:csc[0][2] - 1]))


def test_tier_boundary(esp, model):
    """column 0 with p*q exactly ESP_SPAI_WAVE_DOUBLES (64 x 8) stays with the wave tier, with one more (57 x 9) it is the
    workgroup tier's; both give the model's bits"""
    W = esp._lib.ESP_SPAI_WAVE_DOUBLES
    for (p, q), wide in (((64, 8), 0), ((57, 9), 1)):
        assert p * q == W + wide
        csc = csc_from_columns(sized_columns(p, q), np.random.default_rng(p))
        st, want = check_all(esp, model, from_arrays(esp, csc), arrays=csc)
        assert want.pcol[0] == p and st["max_pq"] == p * q and st["wide"] == wide
        assert np.all(np.isfinite(want.M[2]))


def test_too_large_column_is_refused(esp, model):
    """p*q = ESP_SPAI_DENSE_MAX + 1 (12289 rows, one unknown): ESP_ERR_UNSUPPORTED names the column, p and q; a preconditioner
    updated into that state keeps its earlier M, and serves again once the matrix is one it can take"""
    D = esp._lib.ESP_SPAI_DENSE_MAX
    n = D + 1
    rng = np.random.default_rng(5)
    bad = csc_from_columns(too_large_columns(n), rng)
    with pytest.raises(esp.EspError) as e:
        esp.SPAIPreconditioner(from_arrays(esp, bad))
    assert e.value.code == ESP_ERR_UNSUPPORTED
    msg = str(e.value)
    assert "column 0 " in msg and "p = %d" % n in msg and "q = 1 " in msg and str(D) in msg
    # the same matrix without the rows of column 1 beyond the first three: fine
    good = csc_from_columns([[1], [0, 1, 2]] + [[] for _ in range(2, n)], rng)
    A = from_arrays(esp, good)
    P = Spai(esp, A)
    with np.errstate(all="ignore"):
        want = model.precon(good, 1)
    check_matrix(P, want)
    rows = np.arange(4, n + 1)
    A.append(esp.ESP_UPDATE, rows, np.full(len(rows), 2), np.full(len(rows), 0.5))      # column 1 (1-based 2) grows to every row
    A.flush()
    assert A.nnz() == n + 1
    with pytest.raises(esp.EspError) as e:
        P.update()
    assert e.value.code == ESP_ERR_UNSUPPORTED and "column 0 " in str(e.value)
    cp, rv, nz = P.matrix()                                                             # the earlier M, untouched
    assert np.array_equal(cp, want.M[0]) and np.array_equal(rv, want.M[1]) and same_bits(nz, want.M[2])
    st = P.stats()
    assert (st["max_p"], st["max_q"], st["max_pq"], st["wide"]) == want.stats + (0,)
    with pytest.raises(esp.EspError) as e:
        P.ldiv(np.ones(n))
    assert e.value.code == ESP_ERR_STATE                                                # (A's pattern is no longer M's)
    P.close()


# ---- degenerate columns and special values -----------------------------------------------------------------------------------------
def test_missing_diagonal_and_empty_column(esp, model):
    csc = csc_from_columns([[0, 1], [0, 2], [], [3], [1, 3]], np.random.default_rng(8))
    st, want = check_all(esp, model, from_arrays(esp, csc), arrays=csc)
    assert list(want.pcol) == [3, 2, 0, 1, 3]


def test_rank_deficient_columns(esp, model):
    """two identical columns: the local problem that holds both has an exactly zero pivot; the NaN pattern is the model's"""
    A = np.array([[4.0, 0.0, 0.0, 0.0],
                  [0.0, 2.0, 2.0, 1.0],
                  [0.0, 0.0, 0.0, 1.0],
                  [0.0, 0.0, 0.0, 0.0]])
    st, want = check_all(esp, model, from_scipy(esp, sp.csc_matrix(A)))
    assert np.isnan(want.M[2]).sum() == 2
    B = np.eye(6) * 3.0
    B[1, 0] = B[1, 2] = B[1, 3] = 1.0
    B[:, 4] = B[:, 3]                                   # columns 3 and 4 identical (rows 1 and 3), column 5 holds both
    B[3, 5] = B[4, 5] = 0.5
    check_all(esp, model, from_scipy(esp, sp.csc_matrix(B)))


def test_stored_zeros_and_nan(esp, model):
    """stored 0.0 and -0.0 are entries; one NaN changes exactly the columns whose I x J holds it"""
    A = esp.fdrand(5, 4, 3)
    cp, rv, nz = host_arrays(A)
    clean = model.precon((cp, rv, nz), 1)
    nz2 = nz.copy()
    j0 = 17
    e0 = cp[j0] - 1 + 1                                  # a stored position of column j0
    nz2[[3, 40]] = [0.0, -0.0]
    withzeros = model.precon((cp, rv, nz2), 1)
    nz2[e0] = np.nan
    B = from_arrays(esp, (cp, rv, nz2))
    st, want = check_all(esp, model, B, arrays=(cp, rv, nz2))
    P = esp.SPAIPreconditioner(B)
    got = P.matrix()[2]
    P.close()
    for k in range(len(cp) - 1):
        J = rv[cp[k] - 1:cp[k + 1] - 1] - 1
        col = slice(cp[k] - 1, cp[k + 1] - 1)
        if j0 in J:
            assert np.isnan(got[col]).any()
        else:
            assert same_bits(got[col], withzeros.M[2][col])
    assert not same_bits(withzeros.M[2], clean.M[2])


# ---- update! -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
def test_update_semantics(esp, model, symmetric):
    A = esp.fdrand(5, 4, 3)
    cp, rv, nz = host_arrays(A)
    n = A.n
    lib, h = A._d.lib, A._d.h
    P = Spai(esp, A, 1, symmetric)
    v = np.random.default_rng(2).standard_normal(n)
    u0 = P.ldiv(v)
    # a value change in place without update!: ldiv! is unchanged (M holds results)
    nz2 = nz * (1.0 + 0.25 * np.random.default_rng(3).random(len(nz)))
    if symmetric:                                        # (keep A symmetric)
        S = sp.csc_matrix((nz2, rv - 1, cp - 1), shape=(n, n))
        S = ((S + S.T) * 0.5).tocsc()
        S.sort_indices()
        assert np.array_equal(S.indices + 1, rv)
        nz2 = S.data.copy()
    assert lib.esp_set_nzval(h, vp(nz2)) == 0
    assert same_bits(P.ldiv(v), u0)
    # ... after update! (values only: the kept sizes, tiers and pattern) it equals a fresh create and the model
    P.update()
    want = model.precon((cp, rv, nz2), 1, symmetric)
    check_matrix(P, want)
    F = Spai(esp, A, 1, symmetric)
    check_matrix(F, want)
    assert same_bits(P.ldiv(v), F.ldiv(v)) and same_bits(P.ldiv(v), want.ldiv(v)) and not same_bits(P.ldiv(v), u0)
    F.close()
    # a pattern change without update!: ESP_ERR_STATE; after it a rebuild
    A.append(esp.ESP_UPDATE, [1, n], [n, 1], [-0.125, -0.125])
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.cg(A, v, Pl=P.P), lambda: esp.simple(A, v, Pl=P.P), lambda: esp.gmres(A, v, Pl=P.P),
                 lambda: P.factor()):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    arrays = host_arrays(A)
    assert len(arrays[1]) == len(rv) + 2
    want = model.precon(arrays, 1, symmetric)
    check_matrix(P, want)
    check_ldiv(P, want, seed=4)
    P.close()


def test_order0_update(esp, model):
    A = esp.fdrand(5, 4, 3)
    cp, rv, nz = host_arrays(A)
    P = esp.SPAIPreconditioner(A, 0)
    nz2 = nz * 1.5
    assert A._d.lib.esp_set_nzval(A._d.h, vp(nz2)) == 0
    assert same_bits(P.factor(), model.spai0((cp, rv, nz)))
    P.update()
    assert same_bits(P.factor(), model.spai0((cp, rv, nz2)))
    P.close()


def test_stream_change_between_create_and_update(esp, model):
    hip = C.CDLL("libamdhip64.so")          # (the runtime the library itself is linked against)
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = Spai(esp, A, 1, True)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    A._d.ck(A._d.lib.esp_set_stream(A._d.h, stream))
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.5])
    A.flush()
    P.update()
    want = model.precon(host_arrays(A), 1, True)
    check_matrix(P, want)
    check_ldiv(P, want, seed=6)
    P.close()
    d = A._d
    del A
    d.close()
    assert hip.hipStreamDestroy(stream) == 0


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, order, symmetric):
    p = C.c_void_p()
    rc = lib.esp_precon_spai_create(h, order, symmetric, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for order, symmetric in ((-1, 0), (2, 0), (0, 1)):
        assert raw_create(lib, h, order, symmetric)[0] == ESP_ERR_INVALID
    p = C.c_void_p()
    assert lib.esp_precon_spai_create(None, 1, 0, C.byref(p)) == ESP_ERR_INVALID and lib.esp_precon_spai_create(h, 1, 0, None) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h, 1, 0)[0] == ESP_ERR_INVALID
    one, val = np.ones(1, np.int64), np.ones(1)                                              # pending entries
    assert lib.esp_append_host(h, vp(one), vp(one), vp(val), None, esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h, 1, 0)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # the other kinds' accessors refuse a SPAI preconditioner and the other way round; SPAI is no inner kind
    rc, p, _ = raw_create(lib, h, 1, 0)
    assert rc == 0
    b, path = C.c_void_p(), C.c_int32()
    assert lib.esp_precon_block_matrix(p, C.byref(b), C.byref(path)) == ESP_ERR_INVALID
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 7, C.byref(q)) == ESP_ERR_INVALID
    assert lib.esp_precon_create(h, 0, C.byref(q)) == 0
    out = (C.c_int64 * 4)()
    assert lib.esp_precon_spai_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_spai_matrix(q, C.byref(b)) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(q) == 0
    ptr, idx = np.array([0, 4], np.int64), np.arange(4, dtype=np.int64)
    assert lib.esp_precon_block_create(h, 7, 1, vp(ptr), vp(idx), 0, C.byref(q)) == ESP_ERR_INVALID
    assert lib.esp_precon_colored_create(h, 7, C.byref(q)) == ESP_ERR_INVALID
    # the handle refuses destroy while the preconditioner lives
    assert lib.esp_destroy(h) == ESP_ERR_STATE
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.SPAIPreconditioner(A)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                                       # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, vp(one), vp(one), vp(val), None, esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    rc, _, msg = raw_create(lib, h, 1, 0)
    assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    P.close()


# ---- solvers -----------------------------------------------------------------------------------------------------------------------
def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


def to_device(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg(esp, model, where):
    """the symmetrised SPAI-1 on fdrand 6^3: cg's whole history is the model's; fewer iterations than Jacobi"""
    A = esp.fdrand(6, 6, 6)
    arrays = host_arrays(A)
    b = model.solver.mul(arrays, np.ones(A.n))
    P = esp.SPAIPreconditioner(A, 1, True)
    M = SolverModel(model.solver, model.precon(arrays, 1, True))
    for kw in ({"maxiter": 4}, {"reltol": 1e-8}):
        x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True, **kw)
        wx, wh, wit, wconv = M.cg(b, **kw)
        assert log["iters"] == wit and log["isconverged"] == wconv
        assert same_bits(history_of(log), wh) and same_bits(x if where == "host" else x.cpu().numpy(), wx)
    assert log["isconverged"]
    J = esp.JacobiPreconditioner(A)
    _, jlog = esp.cg(A, b, Pl=J, reltol=1e-8, log=True)
    assert jlog["isconverged"] and log["iters"] < jlog["iters"]
    J.close()
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("order", [0, 1])
def test_nonsymmetric_solvers(esp, model, gmres_lib, where, order):
    """bicgstabl(l = 2), gmres(restart = 20) and simple! on convection-diffusion 4^3 at Pe 4"""
    A = convdiff(esp, 4, 4, 4, 4.0)
    n = A.n
    arrays = host_arrays(A)
    b = model.solver.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.SPAIPreconditioner(A, order)
    M = SolverModel(model.solver, model.precon(arrays, order))
    x, log = esp.bicgstabl(A, dev(b), l=2, Pl=P, log=True)
    wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2)
    assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv) and wconv
    assert same_bits(history_of(log), wh) and same_bits(host(x), wx)
    x, log = esp.gmres(A, dev(b), Pl=P, restart=20, log=True)
    want = gmres_lib.gmres_cb(M, n, b, restart=20)
    assert (log["iters"], log["mvps"], log["reorth"], log["isconverged"]) == (want.iters, want.mvps, want.reorth, want.converged)
    assert want.converged and same_bits(history_of(log), want.history) and same_bits(host(x), want.x)
    u0 = np.random.default_rng(12).standard_normal(n)
    got, log = esp.simple(A, dev(b), u=dev(u0.copy()), Pl=P, maxiter=5, reltol=0.0, log=True)
    wu, wh, wit = M.simple(b, u=u0, maxiter=5, reltol=0.0)
    assert wit == 5 and same_bits(host(got), wu) and same_bits(log["resnorm"], wh)
    P.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    with pytest.raises(ValueError):
        esp.SPAIPreconditioner(A, 2)
    with pytest.raises(ValueError):
        esp.SPAIPreconditioner(A, 0, True)
    with pytest.raises(NotImplementedError):
        esp.AMGCL_RLXPreconditioner(A, type="chebyshev")
    P = esp.AMGCL_RLXPreconditioner(A, type="spai1")
    assert P.order == 1 and not P.symmetric and isinstance(P.stats(), dict) and P.stats()["max_q"] == 7
    b = A.mul(np.ones(A.n))
    for solve in (esp.gmres, esp.bicgstabl):
        assert np.linalg.norm(solve(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    S = esp.SPAIPreconditioner(A, symmetric=True)
    assert S.issymmetric() and np.linalg.norm(esp.cg(A, b, Pl=S) - 1.0) <= 1e-6 * np.sqrt(A.n)
    S.close()
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.SPAIPreconditioner)       # no inner kind of the block preconditioner
    P.close()
    with pytest.raises(ValueError):
        P.ldiv(b)
