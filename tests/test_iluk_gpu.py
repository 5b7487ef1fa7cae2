"""GPU: ILUKPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_iluk_create) against tests/iluk_model.c (the filled
matrix B by the sequential level-of-fill rule) and tests/iluam_model.c applied to that B: B's colptr, rowval, value bits and levels,
the ILUAM factor, ldiv!, the level counts, the solvers' whole histories and the counters of the searches, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from iluam_modellib import level_schedules
from iluk_modellib import Model, parallel_levels
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("iluk_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("iluk_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("iluk_gmres_model"))


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
    """a matrix with exactly S's stored entries (explicit zeros and NaN included), through the CSC constructor"""
    S = sp.csc_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def from_arrays(esp, cp, rv, nz):
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(len(cp) - 1, len(cp) - 1, cp, rv, nz))


def convdiff(esp, nx, ny, nz, pe):
    I, J, V = convdiff_triplets(nx, ny, nz, pe)
    A = esp.ExtendableSparseMatrix(nx * ny * nz, nx * ny * nz)
    A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def check_b(P, want):
    """B and its levels the model's, bit for bit (-0.0 and NaN payloads included)"""
    cp, rv, nz = P.fill_matrix()
    wcp, wrv, wnz = want.B
    assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv)
    assert np.array_equal(bits(nz), bits(wnz))
    assert np.array_equal(P.fill_levels(), want.lev)
    st = P.stats()
    assert st["nnz"] == len(wrv) and st["max_level"] == (int(want.lev.max()) if len(want.lev) else 0)


def check_numeric(P, want, seed=1):
    import torch
    n = want.n
    assert same_bits(P.factor(), want.fval)
    assert P.levels() == tuple(int(l.max()) + 1 for l in level_schedules(want.B[0], want.B[1]))
    v = np.random.default_rng(seed).standard_normal(n)
    u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u)
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


def check_all(esp, model, A, K):
    arrays = host_arrays(A)
    want = model.precon(arrays, K)
    P = esp.ILUKPreconditioner(A, K)
    try:
        assert P.k == K
        check_b(P, want)
        check_numeric(P, want)
        return P.stats(), want
    finally:
        P.close()


# ---- shapes and levels -----------------------------------------------------------------------------------------------------------
def shape(esp, name):
    if name == "n1":
        return from_scipy(esp, sp.csc_matrix(np.array([[4.0]])))
    if name == "n2":
        return from_scipy(esp, sp.csc_matrix(np.array([[4.0, -1.0], [-2.0, 3.0]])))
    if name == "cd6x5x4":
        return convdiff(esp, 6, 5, 4, 2.0)
    return esp.fdrand(*{"fd5x4x3": (5, 4, 3), "fd9x7x1": (9, 7, 1), "fd30x1x1": (30, 1, 1)}[name])


@pytest.mark.parametrize("name", ["n1", "n2", "fd5x4x3", "fd9x7x1", "fd30x1x1", "cd6x5x4"])
@pytest.mark.parametrize("K", [0, 1, 2, 3, 4, "n"])
def test_shapes(esp, model, name, K):
    A = shape(esp, name)
    K = A.n if K == "n" else K
    st, want = check_all(esp, model, A, K)
    if name == "fd30x1x1":                               # a tridiagonal matrix gains nothing
        assert st["nnz"] == A.nnz() and st["max_level"] == 0
    if K == A.n and name in ("fd5x4x3", "cd6x5x4"):      # complete fill: a direct solve (tests/test_iluk_model.py bounds the residual)
        assert st["nnz"] > 4 * A.nnz()


@pytest.mark.parametrize("seed", range(10))
def test_structure_alone_decides(esp, model, seed):
    """structurally non-symmetric patterns, n = 40, about three entries per column and a full diagonal; some stored values are
    0.0, -0.0 and NaN: they count as stored, and their bits are carried into B"""
    n = 40
    rng = np.random.default_rng(100 + seed)
    I = np.concatenate([np.arange(n), rng.integers(0, n, 2 * n)])
    J = np.concatenate([np.arange(n), rng.integers(0, n, 2 * n)])
    S = sp.csc_matrix((np.ones(len(I)), (I, J)), shape=(n, n))
    S.sort_indices()
    cp, rv = S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1
    cols = np.repeat(np.arange(n), np.diff(cp))
    nz = np.where(rv - 1 == cols, 8.0 + rng.random(len(rv)), rng.standard_normal(len(rv)))
    off = np.flatnonzero(rv - 1 != cols)
    for q, s in zip(rng.choice(off, 6, replace=False), [0.0, -0.0, np.nan, 0.0, -0.0, np.nan]):
        nz[q] = s
    A = from_arrays(esp, cp, rv, nz)
    assert np.array_equal(bits(host_arrays(A)[2]), bits(nz))
    for K in (1, 3):
        st, want = check_all(esp, model, A, K)
        assert st["nnz"] > len(rv)


def test_k0_is_iluam(esp, model):
    import torch
    A = esp.fdrand(5, 4, 3)
    P, Q = esp.ILUKPreconditioner(A, 0), esp.ILUAMPreconditioner(A)
    arrays = host_arrays(A)
    cp, rv, nz = P.fill_matrix()
    assert np.array_equal(cp, arrays[0]) and np.array_equal(rv, arrays[1]) and np.array_equal(bits(nz), bits(arrays[2]))
    assert not P.fill_levels().any()
    assert same_bits(P.factor(), Q.factor()) and P.levels() == Q.levels()
    v = np.random.default_rng(3).standard_normal(A.n)
    u = Q.ldiv(v)
    assert same_bits(P.ldiv(v), u)
    t = torch.from_numpy(v.copy()).cuda()
    assert same_bits(P.ldiv(t).cpu().numpy(), u)
    assert P.ldiv(t, out=t).data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    P.close()
    Q.close()


# ---- the tiers of the search -------------------------------------------------------------------------------------------------------
def comb(n, transposed=False, seed=2):
    """a full diagonal, all of column 0 and (0, 1): column 1 fills completely at level 1"""
    rng = np.random.default_rng(seed)
    r = np.arange(1, n)
    I = np.concatenate([np.arange(n), r, [0]])
    J = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64), [1]])
    V = np.concatenate([4.0 + rng.random(n), -0.5 * rng.random(n - 1) - 0.1, [0.75]])
    S = sp.csc_matrix((V, (J, I) if transposed else (I, J)), shape=(n, n))
    S.sort_indices()
    return S


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", ["W-1", "W", "W+1", 5000])
def test_tiers(esp, model, n, transposed):
    """the visited set of column 1 holds all n vertices (itself, column 0 and n - 2 rows of fill): the wave form up to
    ESP_ILUK_WAVE_VISITS, the workgroup form above; n = 5000 puts column 1 of B above the per-column sort's limit"""
    W = esp._lib.ESP_ILUK_WAVE_VISITS
    n = {"W-1": W - 1, "W": W, "W+1": W + 1}.get(n, n)
    A = from_scipy(esp, comb(n, transposed))
    st, want = check_all(esp, model, A, 1)
    assert st["nnz"] == 3 * n - 2 and st["max_level"] == 1
    _, vl, vu = parallel_levels(want.csc[0], want.csc[1], 1)
    assert max(vl + vu) == n
    wide = (sum(v > W for v in vl), sum(v > W for v in vu))
    assert (st["wide_lower"], st["wide_upper"]) == wide
    assert wide == ((0, 0) if n <= W else ((0, 1) if transposed else (1, 0)))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", [4096, 4097])
def test_column_sort_limit(esp, model, n, transposed):
    """the comb at K = 1 with the long line of B at the column sorts' limit, COLSORT_BLOCK = 4096 entries, and one above it.  As it
    stands the line is column 1 of B: 4096 entries are sorted by one workgroup, 4097 go through the flush of a scratch handle.
    Transposed it is row 1 of B (no column holds more than 3 entries) and row 0 of A, whose transpose -- the graph of the upper
    search -- meets the same limit in esp_transpose"""
    A = from_scipy(esp, comb(n, transposed))
    st, want = check_all(esp, model, A, 1)
    cp, rv, _ = want.B
    longest_col, longest_row = int(np.diff(cp).max()), int(np.bincount(rv - 1).max())
    assert (longest_row, longest_col) == ((n, 3) if transposed else (3, n))
    assert st["nnz"] == 3 * n - 2 and st["max_level"] == 1


def test_arrow_fills_completely(esp, model):
    """dense first row and column plus the diagonal, n = 70, K = 1: every position fills, the columns straddle 64 lanes"""
    n = 70
    rng = np.random.default_rng(9)
    r = np.arange(1, n)
    I = np.concatenate([np.arange(n), r, np.zeros(n - 1, np.int64)])
    J = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64), r])
    V = np.concatenate([100.0 + rng.random(n), 0.1 * rng.standard_normal(2 * (n - 1))])
    A = from_scipy(esp, sp.csc_matrix((V, (I, J)), shape=(n, n)))
    st, want = check_all(esp, model, A, 1)
    assert st["nnz"] == n * n and st["max_level"] == 1


def test_beyond_the_widest_search_is_unsupported(esp, model):
    """a comb with n = ESP_ILUK_VISIT_MAX + 3 at K = 1: refused in the count pass, the message names the smallest such column and k;
    A and a preconditioner made before are untouched"""
    n = esp._lib.ESP_ILUK_VISIT_MAX + 3
    A = from_scipy(esp, comb(n))
    before = host_arrays(A)
    P0 = esp.ILUKPreconditioner(A, 0)
    v = np.random.default_rng(4).standard_normal(n)
    u0 = P0.ldiv(v)
    with pytest.raises(esp.EspError) as e:
        esp.ILUKPreconditioner(A, 1)
    assert e.value.code == ESP_ERR_UNSUPPORTED and "column 1 " in str(e.value) and "k = 1" in str(e.value)
    after = host_arrays(A)
    assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
               for a, b in zip(before, after))
    assert same_bits(P0.ldiv(v), u0) and P0.stats()["nnz"] == 2 * n
    P0.update()
    assert same_bits(P0.ldiv(v), u0)
    P0.close()


# ---- updates ---------------------------------------------------------------------------------------------------------------------
def test_values_only_update_equals_fresh_create(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.ILUKPreconditioner(A, 2)
    v = np.random.default_rng(6).standard_normal(n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: the values of the last update!
    for step in (1, 2):
        if step == 2:                                     # updates of stored positions through the buffer and a flush
            d = np.arange(1, n + 1)
            A.append(esp.ESP_UPDATE, d, d, np.full(n, 0.25))
            A.flush()
            assert same_bits(P.ldiv(v), u_new)
        P.update()
        want = model.precon(host_arrays(A), 2)
        F = esp.ILUKPreconditioner(A, 2)
        for Q in (P, F):
            check_b(Q, want)
        u_new = check_numeric(P, want, seed=6)
        assert same_bits(F.ldiv(v), u_new) and not same_bits(u_new, u_old)
        assert same_bits(P.factor(), F.factor())
        F.close()
    P.close()


def test_values_only_update_after_the_scratch_route(esp, model):
    """the comb at n = 4097, K = 1: column 1 of B is above the column sorts' limit, so B, src and the levels come from the flush of a
    scratch handle.  update! with the pattern kept gathers through that src: B is the model's, the factor and ldiv! are bitwise
    those of a preconditioner created afresh"""
    n = 4097
    A = from_scipy(esp, comb(n))
    P = esp.ILUKPreconditioner(A, 1)
    assert int(np.diff(P.fill_matrix()[0]).max()) == n
    v = np.random.default_rng(6).standard_normal(n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    P.update()
    want = model.precon(host_arrays(A), 1)
    F = esp.ILUKPreconditioner(A, 1)
    for Q in (P, F):
        check_b(Q, want)
    u_new = P.ldiv(v)
    assert same_bits(P.factor(), F.factor()) and same_bits(u_new, F.ldiv(v)) and same_bits(u_new, want.ldiv(v))
    assert not same_bits(u_new, u_old)
    F.close()
    P.close()


def test_stream_change_between_create_and_update(esp, model):
    """esp_set_stream on A after the create, then a pattern change: update! moves B's handle and the transpose's to A's new stream
    before it searches, factorizes and solves on them"""
    hip = C.CDLL("libamdhip64.so")          # (the runtime the library itself is linked against)
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.ILUKPreconditioner(A, 1)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    A._d.ck(A._d.lib.esp_set_stream(A._d.h, stream))
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.25])       # two corners: new entries and new fill
    A.flush()
    P.update()
    want = model.precon(host_arrays(A), 1)
    check_b(P, want)
    check_numeric(P, want, seed=6)
    P.close()
    d = A._d
    del A
    d.close()
    assert hip.hipStreamDestroy(stream) == 0


def test_pattern_change_needs_update(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.ILUKPreconditioner(A, 1)
    nnz_b = P.stats()["nnz"]
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.25])       # two corners: new entries and new fill
    A.flush()
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    with pytest.raises(esp.EspError) as e:
        esp.gmres(A, v, Pl=P)
    assert e.value.code == ESP_ERR_STATE
    P.update()
    want = model.precon(host_arrays(A), 1)
    check_b(P, want)
    assert P.stats()["nnz"] > nnz_b + 2
    u = check_numeric(P, want, seed=6)
    F = esp.ILUKPreconditioner(A, 1)
    assert same_bits(F.ldiv(v), u)
    F.close()
    P.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, k):
    p = C.c_void_p()
    rc = lib.esp_precon_iluk_create(h, k, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    assert raw_create(lib, h, -1)[0] == ESP_ERR_INVALID
    p = C.c_void_p()
    assert lib.esp_precon_iluk_create(None, 1, C.byref(p)) == ESP_ERR_INVALID and lib.esp_precon_iluk_create(h, 1, None) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h, 1)[0] == ESP_ERR_INVALID
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))   # no stored (3,3)
    rc, _, msg = raw_create(M._d.lib, M._d.h, 2)
    assert rc == ESP_ERR_INVALID and "diagonal" in msg and "column 3" in msg
    one, val = np.ones(1, np.int64), np.ones(1)                                              # pending entries
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h, 1)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # the other kinds' accessors refuse an ILUK preconditioner and the other way round
    rc, p, _ = raw_create(lib, h, 1)
    assert rc == 0
    b, path = C.c_void_p(), C.c_int32()
    assert lib.esp_precon_block_matrix(p, C.byref(b), C.byref(path)) == ESP_ERR_INVALID
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 2, C.byref(q)) == 0
    out = (C.c_int64 * 4)()
    assert lib.esp_precon_iluk_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_iluk_matrix(q, C.byref(b)) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(q) == 0
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
    P = esp.ILUKPreconditioner(A, 1)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                                       # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    rc, _, msg = raw_create(lib, h, 1)
    assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, v.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_STATE
    P.close()


def test_create_destroy_loop_does_not_leak(esp):
    """the device's free memory, read through the runtime (torch's allocator and the library's own buffers alike), must not keep
    falling over 20 create / update / destroy cycles"""
    import torch
    A = esp.fdrand(20, 20, 20)

    def cycle(k):
        for _ in range(k):
            P = esp.ILUKPreconditioner(A, 1)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(20)
    assert free0 - free1 < (8 << 20), (free0, free1)      # B, its transpose and the ILUAM of 20^3 at k = 1 hold several MiB


# ---- solvers -------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! driven with the ILU(k) model's ldiv and A's mul"""

    def __init__(self, lib, precon):
        self.m, self.P, self.csc, self.n = lib, precon, precon.csc, precon.n

    def ldiv(self, v):
        return self.P.ldiv(np.ascontiguousarray(v, np.float64))


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


def to_device(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg(esp, model, solver_lib, where):
    A = esp.fdrand(5, 4, 3)
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(A.n))
    P = esp.ILUKPreconditioner(A, 1)
    M = SolverModel(solver_lib, model.precon(arrays, 1))
    for kw in ({"maxiter": 4}, {}):
        x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True, **kw)
        wx, wh, wit, wconv = M.cg(b, **kw)
        assert log["iters"] == wit and log["isconverged"] == wconv
        assert same_bits(history_of(log), wh) and same_bits(x if where == "host" else x.cpu().numpy(), wx)
    assert log["isconverged"]
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_nonsymmetric_solvers(esp, model, solver_lib, gmres_lib, where):
    """bicgstabl(l = 2), gmres(restart = 20) and simple! on the convection-diffusion matrix with K = 1"""
    A = convdiff(esp, 6, 5, 4, 2.0)
    n = A.n
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.ILUKPreconditioner(A, 1)
    M = SolverModel(solver_lib, model.precon(arrays, 1))
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


def test_gmres_iterations_fall_with_k(esp, model, solver_lib, gmres_lib):
    """convection-diffusion 12 x 10 x 8, Pe = 4, a seeded right-hand side: the device's iteration counts for K = 0, 1, 2 are the
    model's, and the dial works: fewer iterations at K = 2 than at K = 0"""
    A = convdiff(esp, 12, 10, 8, 4.0)
    n = A.n
    arrays = host_arrays(A)
    b = np.random.default_rng(9).standard_normal(n)
    iters, ratio = [], []
    for K in (0, 1, 2):
        P = esp.ILUKPreconditioner(A, K)
        want = gmres_lib.gmres_cb(SolverModel(solver_lib, model.precon(arrays, K)), n, b, restart=20)
        x, log = esp.gmres(A, b, Pl=P, restart=20, log=True)
        assert log["iters"] == want.iters and log["isconverged"] and want.converged
        assert same_bits(history_of(log), want.history) and same_bits(x, want.x)
        iters.append(want.iters)
        ratio.append(P.stats()["nnz"] / A.nnz())
        P.close()
    print("gmres(restart=20) iterations for K = 0, 1, 2:", iters, "nnz(B)/nnz(A):", ["%.2f" % r for r in ratio])
    assert iters[2] < iters[0]


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    with pytest.raises(ValueError):
        esp.ILUKPreconditioner(A, -1)
    with pytest.raises(ValueError):
        esp.ILUKPreconditioner(A, 1.5)
    P = esp.ILUKPreconditioner(A)
    assert P.k == 1 and isinstance(P.stats(), dict)
    b = A.mul(np.ones(A.n))
    for solve in (esp.cg, esp.gmres, esp.bicgstabl):
        assert np.linalg.norm(solve(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    assert np.linalg.norm(esp.simple(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.ILUKPreconditioner)       # no inner kind of the block preconditioner
    D = esp.ILUKPreconditioner(A, A.n)                                                # complete fill: a direct solve
    assert np.linalg.norm(D.ldiv(b) - 1.0) <= 1e-12 * np.sqrt(A.n)
    D.close()
    P.close()
    with pytest.raises(ValueError):
        P.ldiv(b)
