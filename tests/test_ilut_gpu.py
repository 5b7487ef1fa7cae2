"""GPU: ILUTPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_ilut_create) against tests/ilut_model.c, bit for bit:
the pattern S, the factors F, the per-step counts, the tiers of the sweep kernel, ldiv! (iluam_model.c over (S, F)), the level
counts, the updates with and without keep_pattern and the solvers' whole histories."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from iluam_modellib import level_schedules
from ilut_modellib import FillRefused, Model
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("ilut_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("ilut_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("ilut_gmres_model"))


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


def tier_counts(esp, S):
    """the columns of S by the rows above their diagonal: (wave, group, stride)"""
    cp, rv = S
    n = len(cp) - 1
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    up = np.bincount(cols[rv < cols] - 1, minlength=n) if n else np.zeros(0, np.int64)
    W, G = esp._lib.ESP_ILUT_WAVE_UPPER, esp._lib.ESP_ILUT_GROUP_UPPER
    return int((up <= W).sum()), int(((up > W) & (up <= G)).sum()), int((up > G).sum())


def check_state(esp, P, want):
    """S, F, the counts and the tiers the model's, bit for bit"""
    cp, rv, nz = P.matrix()
    assert np.array_equal(cp, want.S[0]) and np.array_equal(rv, want.S[1])
    assert same_bits(nz, want.F) and same_bits(P.factor(), want.F)
    st = P.stats()
    assert st["nnz"] == len(want.S[1]) and st["steps"] == want.stats and st["sweeps"] == want.sweeps_run
    assert (st["wave"], st["group"], st["stride"]) == tier_counts(esp, want.S)
    lev = level_schedules(want.S[0], want.S[1])
    assert P.levels() == (0,) + tuple(int(l.max()) + 1 if len(l) else 0 for l in lev[1:])


def check_ldiv(P, want, seed=1):
    import torch
    v = np.random.default_rng(seed).standard_normal(want.n)
    with np.errstate(all="ignore"):
        u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u)
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


def check_all(esp, model, A, *par, **kw):
    with np.errstate(all="ignore"):
        want = model.precon(host_arrays(A), *par, **kw)
    P = esp.ILUTPreconditioner(A, *par, **kw)
    try:
        check_state(esp, P, want)
        check_ldiv(P, want)
        return P.stats(), want
    finally:
        P.close()


# ---- shapes, tolerances and steps --------------------------------------------------------------------------------------------------
def shape(esp, name):
    if name == "n1":
        return from_scipy(esp, sp.csc_matrix(np.array([[4.0]])))
    if name == "n2":
        return from_scipy(esp, sp.csc_matrix(np.array([[4.0, -1.0], [-2.0, 3.0]])))
    if name == "cd6x5x4":
        return convdiff(esp, 6, 5, 4, 2.0)
    return esp.fdrand(*{"fd5x4x3": (5, 4, 3), "fd9x7x1": (9, 7, 1), "fd30x1x1": (30, 1, 1)}[name])


@pytest.mark.parametrize("name", ["n1", "n2", "fd5x4x3", "fd9x7x1", "fd30x1x1", "cd6x5x4"])
@pytest.mark.parametrize("tau", [0.0, 1e-3, 1e-2, 0.3])
@pytest.mark.parametrize("steps", [0, 1, 3])
def test_shapes(esp, model, name, tau, steps):
    A = shape(esp, name)
    st, want = check_all(esp, model, A, tau, steps, 3)
    if steps == 0 or name == "fd30x1x1":                 # a tridiagonal matrix has no candidates beyond itself
        assert st["nnz"] <= A.nnz()
    if tau == 0.0 and steps == 3 and name in ("fd5x4x3", "cd6x5x4"):
        assert st["nnz"] > 2 * A.nnz()


@pytest.mark.parametrize("seed", range(10))
def test_random_patterns(esp, model, seed):
    """structurally non-symmetric patterns, n = 40, about three entries per column and a full dominant diagonal"""
    n = 40
    rng = np.random.default_rng(200 + seed)
    I = np.concatenate([np.arange(n), rng.integers(0, n, 2 * n)])
    J = np.concatenate([np.arange(n), rng.integers(0, n, 2 * n)])
    S = sp.csc_matrix((np.ones(len(I)), (I, J)), shape=(n, n))
    S.sort_indices()
    cp, rv = S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1
    cols = np.repeat(np.arange(n), np.diff(cp))
    nz = np.where(rv - 1 == cols, 8.0 + rng.random(len(rv)), rng.standard_normal(len(rv)))
    A = from_arrays(esp, cp, rv, nz)
    for tau, steps, sweeps in ((1e-2, 1, 2), (1e-3, 3, 3), (0.0, 2, 1)):
        st, want = check_all(esp, model, A, tau, steps, sweeps)
    assert st["nnz"] > len(rv)


def test_fixed_point_is_iluam(esp, model):
    """steps = 0 and 2n sweeps: the values no longer change and are ILUAMPreconditioner's factorization, bit for bit -- the new
    kernel against code that is pinned already"""
    A = esp.fdrand(5, 4, 3)
    P, Q = esp.ILUTPreconditioner(A, steps=0, sweeps=2 * A.n), esp.ILUAMPreconditioner(A)
    cp, rv, nz = P.matrix()
    arrays = host_arrays(A)
    assert np.array_equal(cp, arrays[0]) and np.array_equal(rv, arrays[1])
    assert same_bits(P.factor(), Q.factor()) and same_bits(nz, Q.factor())
    v = np.random.default_rng(3).standard_normal(A.n)
    assert same_bits(P.ldiv(v), Q.ldiv(v)) and P.levels()[1:] == Q.levels()[1:]
    P.close()
    Q.close()


@pytest.mark.parametrize("keep", [False, True])
def test_empty_matrix(esp, keep):
    A = esp.ExtendableSparseMatrix(0, 0)
    P = esp.ILUTPreconditioner(A, keep_pattern=keep)
    st = P.stats()
    assert st["nnz"] == 0 and (st["wave"], st["group"], st["stride"]) == (0, 0, 0)
    assert len(P.ldiv(np.zeros(0))) == 0
    x, log = esp.cg(A, np.zeros(0), Pl=P, log=True)
    assert log["iters"] == 0 and log["isconverged"]
    P.update()
    P.close()


# ---- the tiers of the sweep kernel ---------------------------------------------------------------------------------------------------
def long_line(n, transposed, seed=2):
    """tridiagonal plus a full last column (transposed: a full last row): the last column holds n - 1 rows above its diagonal, and
    every one of its entries merges a row against them; no position fills"""
    rng = np.random.default_rng(seed)
    r = np.arange(n - 1)
    I = np.concatenate([np.arange(n), r + 1, r, r[:-1]])
    J = np.concatenate([np.arange(n), r, r + 1, np.full(n - 2, n - 1)])
    V = np.concatenate([4.0 + rng.random(n), -0.5 * rng.random(n - 1) - 0.1, -0.5 * rng.random(n - 1) - 0.1, 0.1 * rng.standard_normal(n - 2)])
    S = sp.csc_matrix((V, (J, I) if transposed else (I, J)), shape=(n, n))
    S.sort_indices()
    return S


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("cap", ["wave", "group"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tiers(esp, model, cap, delta, transposed):
    """the rows above the last column's diagonal at each tier's cap - 1, cap and cap + 1; transposed the long line is a row, which
    every tier merges against short columns"""
    lim = (C.c_int64 * 4)()
    assert esp._lib.load().esp_precon_ilut_limits(lim) == 0
    assert (lim[0], lim[1]) == (esp._lib.ESP_ILUT_WAVE_UPPER, esp._lib.ESP_ILUT_GROUP_UPPER)
    up = {"wave": lim[0], "group": lim[1]}[cap] + delta
    n = up + 1
    A = from_scipy(esp, long_line(n, transposed))
    st, want = check_all(esp, model, A, 0.0, 1, 2)
    assert st["nnz"] == A.nnz() == 4 * n - 4
    if transposed:
        assert (st["group"], st["stride"]) == (0, 0)
    else:
        assert (st["group"], st["stride"]) == ((0, 0) if up <= lim[0] else (1, 0) if up <= lim[1] else (0, 1))


# ---- special values ----------------------------------------------------------------------------------------------------------------
def test_stored_zero_nan_and_zero_pivot(esp, model):
    """a stored 0.0 / -0.0 counts as stored; NaN and Inf propagate (a zero pivot divides): no error, the model's bits"""
    A0 = esp.fdrand(5, 4, 3)
    cp, rv, nz = host_arrays(A0)
    n = A0.n
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    off = np.flatnonzero(rv != cols)
    for kind in ("zeros", "nan", "pivot"):
        v = nz.copy()
        if kind == "zeros":
            v[off[[2, 11, 40]]] = [0.0, -0.0, 0.0]
        elif kind == "nan":
            v[off[7]] = np.nan
        else:
            v[np.flatnonzero(rv == cols)[4]] = 0.0
        A = from_arrays(esp, cp, rv, v)
        for tau, steps in ((1e-2, 2), (0.0, 1)):
            st, want = check_all(esp, model, A, tau, steps, 2)
        if kind != "zeros":
            assert not np.isfinite(want.F).all()


def test_a_column_left_with_its_diagonal_alone(esp, model):
    M = np.array([[4.0, 1e-6, 1.0, 0.0], [1e-6, 5.0, 0.0, 1e-6], [1.0, 0.0, 6.0, 1.0], [0.0, 1e-6, 1.0, 7.0]])
    A = from_scipy(esp, sp.csc_matrix(M))
    st, want = check_all(esp, model, A, 1e-3, 2, 2)
    lens = np.diff(want.S[0])
    assert lens[1] == 1 and lens.max() > 1


# ---- updates ---------------------------------------------------------------------------------------------------------------------
def perturb(A, seed):
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(seed).random(len(csc.nzval)))
    A._push_edits()


@pytest.mark.parametrize("keep", [False, True])
def test_values_only_update(esp, model, keep):
    """keep_pattern False: the construction again (a fresh create's result); True: the pattern stays and the sweeps start from the
    current F -- twice in a row -- which is the model's carried state and not a fresh create's"""
    A = esp.fdrand(5, 4, 3)
    par = dict(droptol=1e-2, steps=2, sweeps=2, keep_pattern=keep)
    P = esp.ILUTPreconditioner(A, **par)
    want = model.precon(host_arrays(A), **par)
    check_state(esp, P, want)
    v = np.random.default_rng(6).standard_normal(A.n)
    u_old = P.ldiv(v)
    for seed in (8, 9):
        perturb(A, seed)
        assert same_bits(P.ldiv(v), u_old)                # no update!: the values of the last update!
        P.update()
        want.update(host_arrays(A))
        check_state(esp, P, want)
        u_new = check_ldiv(P, want, seed=6)
        assert not same_bits(u_new, u_old)
        F = esp.ILUTPreconditioner(A, **par)
        assert same_bits(F.factor(), P.factor()) == (not keep)       # (warm: the carried state is no fresh create's)
        F.close()
        u_old = u_new
    assert P.stats()["sweeps"] == (2 if keep else 8)
    P.close()


@pytest.mark.parametrize("keep", [False, True])
def test_update_after_a_pattern_change(esp, model, keep):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    par = dict(droptol=1e-3, steps=1, sweeps=2, keep_pattern=keep)
    P = esp.ILUTPreconditioner(A, **par)
    want = model.precon(host_arrays(A), **par)
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.25])       # two corners: new entries and new candidates
    A.flush()
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    with pytest.raises(esp.EspError) as e:
        esp.gmres(A, v, Pl=P)
    assert e.value.code == ESP_ERR_STATE
    P.update()
    want.update(host_arrays(A))
    check_state(esp, P, want)
    check_ldiv(P, want, seed=6)
    fresh = model.precon(host_arrays(A), **par)
    assert same_bits(want.F, fresh.F)                            # a pattern change: the whole construction, keep_pattern or not
    P.close()


def test_stream_change_between_create_and_update(esp, model):
    """esp_set_stream on A after the create: update! moves F's handle and the work handles to A's new stream first"""
    hip = C.CDLL("libamdhip64.so")          # (the runtime the library itself is linked against)
    A = esp.fdrand(5, 4, 3)
    P = esp.ILUTPreconditioner(A, 1e-2, 2, 2, keep_pattern=True)
    want = model.precon(host_arrays(A), 1e-2, 2, 2, keep_pattern=True)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    A._d.ck(A._d.lib.esp_set_stream(A._d.h, stream))
    perturb(A, 8)
    P.update()                                                   # warm, on the new stream
    want.update(host_arrays(A))
    check_state(esp, P, want)
    A.append(esp.ESP_UPDATE, [A.n, 1], [1, A.n], [0.5, 0.25])
    A.flush()
    P.update()                                                   # the whole construction, on the new stream
    want.update(host_arrays(A))
    check_state(esp, P, want)
    check_ldiv(P, want, seed=6)
    P.close()
    d = A._d
    del A
    d.close()
    assert hip.hipStreamDestroy(stream) == 0


def test_fill_guard_leaves_the_previous_factorization(esp, model):
    """with tiny off-diagonal values step 0 drops everything and step 1 has few candidates; max_fill is set just above them.  With
    the off-diagonal values large nothing is dropped, step 1 exceeds the limit and update! refuses: the message names the step and
    both counts, and ldiv! still applies the factorization of the last good update!"""
    A = esp.fdrand(5, 4, 3)
    cp, rv, nz = host_arrays(A)
    n, nnz = A.n, A.nnz()
    diag = rv == np.repeat(np.arange(1, n + 1), np.diff(cp))
    small, large = np.where(diag, nz, 1e-4 * nz), nz

    def set_values(v):
        csc = A.sparse()
        csc.nzval[:] = v
        A._push_edits()
    c0, c1 = model.precon((cp, rv, large), 0.05, 2, 1, max_fill=1e6).stats[1][0], model.precon((cp, rv, small), 0.05, 2, 1, max_fill=1e6).stats
    limit = max(c1[0][0], c1[1][0])
    assert c0 > limit
    par = dict(droptol=0.05, steps=2, sweeps=1, max_fill=(limit + 0.5) / nnz)
    set_values(small)
    P = esp.ILUTPreconditioner(A, **par)
    want = model.precon((cp, rv, small), **par)
    check_state(esp, P, want)
    v = np.random.default_rng(6).standard_normal(n)
    u = P.ldiv(v)
    set_values(large)
    with pytest.raises(FillRefused) as m:
        want.update((cp, rv, large))
    assert (m.value.step, m.value.nnz_c, m.value.limit) == (1, c0, limit)
    with pytest.raises(esp.EspError) as e:
        P.update()
    assert e.value.code == ESP_ERR_UNSUPPORTED
    assert "step 1" in str(e.value) and str(c0) in str(e.value) and str(limit) in str(e.value)
    assert same_bits(P.ldiv(v), u)
    check_state(esp, P, want)
    set_values(small * 1.25)
    P.update()
    want.update((cp, rv, small * 1.25))
    check_state(esp, P, want)
    check_ldiv(P, want)
    P.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, tau=1e-3, steps=3, sweeps=3, max_fill=32.0, keep=0):
    p = C.c_void_p()
    rc = lib.esp_precon_ilut_create(h, tau, steps, sweeps, max_fill, keep, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for kw in ({"tau": -1e-3}, {"tau": float("nan")}, {"steps": -1}, {"steps": 17}, {"sweeps": 0}, {"max_fill": 0.5}, {"max_fill": float("nan")}):
        assert raw_create(lib, h, **kw)[0] == ESP_ERR_INVALID, kw
    p = C.c_void_p()
    assert lib.esp_precon_ilut_create(None, 1e-3, 3, 3, 32.0, 0, C.byref(p)) == ESP_ERR_INVALID
    assert lib.esp_precon_ilut_create(h, 1e-3, 3, 3, 32.0, 0, None) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h)[0] == ESP_ERR_INVALID
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))   # no stored (3,3)
    rc, _, msg = raw_create(M._d.lib, M._d.h)
    assert rc == ESP_ERR_INVALID and "diagonal" in msg and "column 3" in msg
    one, val = np.ones(1, np.int64), np.ones(1)                                              # pending entries
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # the other kinds' accessors refuse an ILUT preconditioner and the other way round
    rc, p, _ = raw_create(lib, h, steps=16)
    assert rc == 0
    b = C.c_void_p()
    assert lib.esp_precon_iluk_matrix(p, C.byref(b)) == ESP_ERR_INVALID
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 2, C.byref(q)) == 0
    out = (C.c_int64 * 40)()
    assert lib.esp_precon_ilut_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_ilut_matrix(q, C.byref(b)) == ESP_ERR_INVALID
    assert lib.esp_precon_ilut_stats(p, None) == ESP_ERR_INVALID and lib.esp_precon_ilut_limits(None) == ESP_ERR_INVALID
    assert lib.esp_precon_ilut_stats(p, out) == 0 and out[0] == 16
    assert lib.esp_precon_destroy(q) == 0
    assert lib.esp_destroy(h) == ESP_ERR_STATE                   # the handle refuses destroy while the preconditioner lives
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.ILUTPreconditioner(A)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                                       # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    rc, _, msg = raw_create(lib, h)
    assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, v.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_STATE
    P.close()


def test_create_destroy_loop_does_not_leak(esp):
    """the device's free memory, read through the runtime, must not keep falling over 20 create / update / destroy cycles"""
    import torch
    A = esp.fdrand(16, 16, 16)

    def cycle(k):
        for _ in range(k):
            P = esp.ILUTPreconditioner(A, 1e-2, 2, 2, keep_pattern=True)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(20)
    assert free0 - free1 < (8 << 20), (free0, free1)


# ---- solvers -------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! driven with the ILUT model's ldiv and A's mul"""

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
    P = esp.ILUTPreconditioner(A, 1e-2)
    M = SolverModel(solver_lib, model.precon(arrays, 1e-2))
    for kw in ({"maxiter": 3}, {}):
        x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True, **kw)
        wx, wh, wit, wconv = M.cg(b, **kw)
        assert log["iters"] == wit and log["isconverged"] == wconv
        assert same_bits(history_of(log), wh) and same_bits(x if where == "host" else x.cpu().numpy(), wx)
    assert log["isconverged"]
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_nonsymmetric_solvers(esp, model, solver_lib, gmres_lib, where):
    """bicgstabl(l = 2), gmres(restart = 20) and simple! on the convection-diffusion matrix"""
    A = convdiff(esp, 6, 5, 4, 2.0)
    n = A.n
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.ILUTPreconditioner(A, 1e-2)
    M = SolverModel(solver_lib, model.precon(arrays, 1e-2))
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


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    for bad in ({"droptol": -1.0}, {"droptol": float("nan")}, {"steps": -1}, {"steps": 17}, {"steps": 1.5}, {"sweeps": 0}, {"max_fill": 0.5}):
        with pytest.raises(ValueError):
            esp.ILUTPreconditioner(A, **bad)
    P = esp.ILUTPreconditioner(A)
    assert (P.droptol, P.steps, P.sweeps, P.max_fill, P.keep_pattern) == (1e-3, 3, 3, 32.0, False)
    st = P.stats()
    assert len(st["steps"]) == 3 and st["sweeps"] == 18 and st["nnz"] == len(P.factor()) == len(P.matrix()[1])
    b = A.mul(np.ones(A.n))
    for solve in (esp.cg, esp.gmres, esp.bicgstabl):
        assert np.linalg.norm(solve(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    assert np.linalg.norm(esp.simple(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    for outer in (lambda: esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.ILUTPreconditioner),
                  lambda: esp.ColoredPreconditioner(A, esp.ILUTPreconditioner)):
        with pytest.raises(TypeError):                               # no inner kind of Block or Colored
            outer()
    Q = esp.AMGCL_RLXPreconditioner(A, type="ilut")
    assert isinstance(Q, esp.ILUTPreconditioner) and same_bits(Q.factor(), P.factor())
    with pytest.raises(NotImplementedError):
        esp.AMGCL_RLXPreconditioner(A, type="chebyshev")
    Q.close()
    P.close()
    with pytest.raises(ValueError):
        P.ldiv(b)
