"""GPU: AMGPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_amg_create) against the model of
tests/amg_modellib.py (amg_model.c is normative): aggregates, Luby rounds and root counts of every level, every P_l and A_l,
rho_l, the coarsest level's inverse, ldiv! and x with the whole residual history of cg, bicgstabl and simple! bit for bit (a NaN
equals a NaN at the same position: its payload is not pinned); the error table; and the reference's own acceptance test of its
AMG kinds (test/test_preconditioners.jl:10-20,41) replayed on top."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import amg_modellib as am
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_NOMEM, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -4, -5, -6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return am.Model(tmp_path_factory.mktemp("amg_model"))


@pytest.fixture(scope="module")
def fd(orc):
    cache = {}

    def get(*dims):
        if dims not in cache:
            O = orc.fdrand(*dims, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
            cache[dims] = tuple(np.array(a) for a in O.sparse().arrays())
        return cache[dims]
    return get


@pytest.fixture(scope="module")
def graphs(fd):
    return am.graphs(fd)


@pytest.fixture(scope="module")
def m20(model, fd):
    """the model hierarchy of fdrand 20 x 20 x 20 with the defaults: computed once, shared, left unchanged"""
    return am.AMGModel(model, fd(20, 20, 20))


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def matrix(esp, csc):
    cp, rv, nz = csc
    n = len(cp) - 1
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, np.array(cp, np.int64), np.array(rv, np.int64), np.array(nz, np.float64)))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def check_hierarchy(P, M):
    assert P.levels == len(M.levels)
    for l, L in enumerate(M.levels):
        D = P.level(l)
        assert D["n"] == L.n and D["rounds"] == L.rounds, l
        assert same_bits([D["rho"]], [L.rho]), (l, D["rho"], L.rho)
        for got, want in ((D["A"], L.A), (D["P"], L.P)):
            assert (got is None) == (want is None), l
            if want is not None:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), l
                assert same_bits(got[2], want[2]), l
        if L.agg is not None:
            agg = P.aggregates(l)
            assert np.array_equal(agg, L.agg), l
            assert (agg.max() + 1 if L.n else 0) == L.nc                   # the root count
            if L.P is not None:
                assert M.levels[l + 1].n == L.nc
        else:
            with pytest.raises(Exception):
                P.aggregates(l)
    if M.inv is not None:
        assert same_bits(P.coarse_inverse(), M.inv)
    else:
        with pytest.raises(Exception):
            P.coarse_inverse()


def check_ldiv(P, M, seed=1):
    """host vectors, device vectors, in place on both sides"""
    import torch
    n = M.n
    v = np.random.default_rng(seed).standard_normal(n)
    with np.errstate(all="ignore"):
        want = M.ldiv(v)
    assert same_bits(P.ldiv(v), want)
    if n == 0:
        return want
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t)
    assert same_bits(out.cpu().numpy(), want) and same_bits(t.cpu().numpy(), v)
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), want)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, want)
    return want


def check_all(esp, model, csc, **kw):
    A = matrix(esp, csc)
    P = esp.AMGPreconditioner(A, **kw)
    try:
        with np.errstate(all="ignore"):
            M = am.AMGModel(model, csc, **kw)
        check_hierarchy(P, M)
        check_ldiv(P, M)
        return M
    finally:
        P.close()


# ---- aggregates, rounds, root counts and the whole hierarchy on the graphs of the issue ------------------------------------------
@pytest.mark.parametrize("name", am.GRAPH_NAMES)
def test_aggregation_and_hierarchy(esp, model, graphs, name):
    """max_coarse = 1: every level with more than one unknown is aggregated, until one unknown is left or the aggregation stalls"""
    csc, theta = graphs[name]
    M = check_all(esp, model, csc, max_coarse=1, theta=theta)
    n = len(csc[0]) - 1
    if n > 1:
        assert M.levels[0].agg is not None and M.levels[0].rounds >= 1
    if name.startswith("star"):
        assert np.diff(csc[0]).max() == n and [L.n for L in M.levels] == [n, 1]        # the hub's column: the whole-wave path


def test_default_parameters_and_the_alias(esp, model, fd):
    csc = fd(5, 5, 5)
    A = matrix(esp, csc)
    lib, h = A._d.lib, A._d.h
    p = C.c_void_p()
    assert lib.esp_precon_amg_create(h, -1, -1, -1, -1, -1.0, C.byref(p)) == 0      # -1 / a negative theta: the defaults
    M = am.AMGModel(model, csc)
    v = np.random.default_rng(3).standard_normal(A.n)
    u = np.empty_like(v)
    assert lib.esp_precon_ldiv(p, vp(v), vp(u), 0) == 0 and same_bits(u, M.ldiv(v))
    out = (C.c_int64 * 3)(7, 7, 7)
    assert lib.esp_precon_levels(p, out) == 0 and list(out) == [0, 0, 0]
    assert lib.esp_precon_get_factor(p, vp(u), 0) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(p) == 0
    P = esp.SA_AMGPreconditioner(A)
    check_hierarchy(P, M)
    P.close()


def test_inspection_into_device_memory(esp, model, fd):
    import torch
    csc = fd(7, 6, 5)
    A = matrix(esp, csc)
    P = esp.AMGPreconditioner(A)
    M = am.AMGModel(model, csc)
    lib = A._d.lib
    agg = torch.full((A.n,), -7, dtype=torch.int64, device="cuda")
    nl = M.levels[-1].n
    inv = torch.zeros(nl * nl, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert lib.esp_precon_amg_aggregates(P._p, 0, C.c_void_p(agg.data_ptr()), 1) == 0
    assert lib.esp_precon_amg_coarse_inverse(P._p, C.c_void_p(inv.data_ptr()), 1) == 0
    assert np.array_equal(agg.cpu().numpy(), M.levels[0].agg) and same_bits(inv.cpu().numpy().reshape(nl, nl), M.inv)
    assert lib.esp_precon_amg_aggregates(P._p, P.levels - 1, C.c_void_p(agg.data_ptr()), 1) == ESP_ERR_INVALID     # not aggregated
    assert lib.esp_precon_amg_aggregates(P._p, P.levels, C.c_void_p(agg.data_ptr()), 1) == ESP_ERR_INVALID         # no such level
    assert lib.esp_precon_amg_level(P._p, -1, None, None, None, None, None) == ESP_ERR_INVALID
    P.close()


def test_hierarchy_keeps_an_explicit_zero_a_negative_zero_and_a_nan(esp, model, fd):
    cp, rv, nz = (np.array(a, copy=True) for a in fd(6, 5, 4))
    n = len(cp) - 1

    def pos(i, j):
        k = cp[j] - 1 + np.searchsorted(rv[cp[j] - 1:cp[j + 1] - 1], i + 1)
        assert rv[k] == i + 1
        return k
    nz[pos(0, 1)] = nz[pos(1, 0)] = 0.0          # a stored zero pair: no edge
    nz[pos(7, 13)] = -0.0                        # one side -0.0: still an edge
    nz[pos(50, 56)] = np.nan                     # a NaN: it spreads through the Galerkin products
    check_all(esp, model, (cp, rv, nz), max_coarse=8)


# ---- the coarsest level -------------------------------------------------------------------------------------------------------------
def full_csc(a):
    n = a.shape[0]
    return 1 + n * np.arange(n + 1, dtype=np.int64), np.tile(np.arange(1, n + 1, dtype=np.int64), n), np.ascontiguousarray(a.T).reshape(-1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_coarse_inverse_direct(esp, model, n):
    """max_levels = 1: the matrix itself is inverted"""
    a = np.random.default_rng(n).standard_normal((n, n)) + n * np.eye(n)
    M = check_all(esp, model, full_csc(a), max_levels=1, max_coarse=1)
    assert len(M.levels) == 1 and M.inv.shape == (n, n)
    assert np.abs(M.inv @ a - np.eye(n)).max() < 1e-12


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_coarse_inverse_below_a_fine_level(esp, model, n):
    """a path whose first aggregation leaves exactly n unknowns, max_coarse = n: the hierarchy stops there"""
    size = {1: 2, 2: 5}.get(n)
    if size is None:
        for size in range(2 * n, 6 * n):
            st = model.strength(am.path_graph(size), 0.0)
            if model.aggregate(am.path_graph(size), st)[1] == n:
                break
    M = check_all(esp, model, am.path_graph(size), max_coarse=n)
    assert [L.n for L in M.levels] == [size, n] and M.inv.shape == (n, n)


def test_coarse_inverse_row_swap_and_zero_pivot(esp, model):
    swap = np.array([[0.0, 2.0, 1.0], [4.0, 1.0, 0.0], [-4.0, 3.0, 5.0]])       # a stored zero diagonal; |4| == |-4|
    M = check_all(esp, model, full_csc(swap), max_levels=1)
    assert np.abs(M.inv @ swap - np.eye(3)).max() < 1e-14
    M = check_all(esp, model, full_csc(np.array([[1.0, 2.0], [2.0, 4.0]])), max_levels=1)      # a zero pivot is no error
    assert not np.isfinite(M.inv).all()                                          # (Inf and NaN compared by position)


def test_smoothing_only_coarsest(esp, model):
    """a diagonal matrix of 600 unknowns: no strong edges, n_1 == n_0 > 512"""
    n = 600
    csc = (np.arange(1, n + 2, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64), 1.0 + np.arange(n) / n)
    M = check_all(esp, model, csc)
    assert len(M.levels) == 1 and M.inv is None and M.levels[0].nc == n and M.levels[0].rounds == 1


# ---- ldiv! ----------------------------------------------------------------------------------------------------------------------------
def test_ldiv_5x5x5(esp, model, fd):
    M = check_all(esp, model, fd(5, 5, 5))
    assert len(M.levels) == 2


def test_ldiv_20_cubed_defaults(esp, model, fd, m20):
    A = matrix(esp, fd(20, 20, 20))
    P = esp.AMGPreconditioner(A)
    check_hierarchy(P, m20)
    check_ldiv(P, m20)
    assert len(m20.levels) >= 3
    P.close()


@pytest.mark.parametrize("sweeps", [(2, 2), (1, 0), (3, 1)])
def test_ldiv_sweeps(esp, model, fd, sweeps):
    check_all(esp, model, fd(20, 20, 20), presweeps=sweeps[0], postsweeps=sweeps[1])


@pytest.mark.parametrize("max_levels", [1, 2, 10])
def test_ldiv_max_levels(esp, model, fd, max_levels):
    M = check_all(esp, model, fd(20, 20, 20), max_levels=max_levels)
    assert len(M.levels) == min(max_levels, 3)
    assert (M.inv is None) == (max_levels < 3)            # 8000 and its first coarse level exceed 512: smoothed only


# ---- the solvers with Pl = AMG: x and the whole residual history ------------------------------------------------------------------
def test_cg_with_amg(esp, model, fd):
    import torch
    csc = fd(9, 8, 7)
    A = matrix(esp, csc)
    P = esp.AMGPreconditioner(A)
    M = am.AMGModel(model, csc)
    b = np.ones(A.n)
    wx, wh, wit, wconv = M.cg(b, reltol=1e-8)
    x, log = esp.cg(A, b, Pl=P, reltol=1e-8, log=True)
    assert log["iters"] == wit and log["isconverged"] == wconv and wconv
    assert same_bits(x, wx) and same_bits(np.concatenate([[log["r0"]], log["resnorm"]]), wh)
    t = torch.from_numpy(b).cuda()
    xt, log = esp.cg(A, t, Pl=P, reltol=1e-8, maxiter=5, log=True)
    wx, wh, wit, _ = M.cg(b, reltol=1e-8, maxiter=5)
    assert log["iters"] == wit == 5 and same_bits(xt.cpu().numpy(), wx) and same_bits(log["resnorm"], wh[1:])
    P.close()


def test_bicgstabl_with_amg_on_convection_diffusion(esp, model):
    csc = am.convdiff(8, 7, 3, 2.0)
    A = matrix(esp, csc)
    for kw in ({}, {"theta": 0.25}):
        P = esp.AMGPreconditioner(A, **kw)
        M = am.AMGModel(model, csc, **kw)
        check_hierarchy(P, M)
        b = np.random.default_rng(9).standard_normal(A.n)
        wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2, reltol=1e-8)
        x, log = esp.bicgstabl(A, b, l=2, Pl=P, reltol=1e-8, log=True)
        assert log["iters"] == wit and log["mvps"] == wmv and log["isconverged"] == wconv and wconv
        assert same_bits(x, wx) and same_bits(np.concatenate([[log["r0"]], log["resnorm"]]), wh)
        P.close()


def test_simple_with_amg(esp, model, fd):
    import torch
    csc = fd(9, 8, 7)
    A = matrix(esp, csc)
    P = esp.AMGPreconditioner(A)
    M = am.AMGModel(model, csc)
    b = np.ones(A.n)
    wu, wh, wit = M.simple(b, maxiter=40, reltol=1e-6)
    u, log = esp.simple(A, b, Pl=P, maxiter=40, reltol=1e-6, log=True)
    assert len(log["resnorm"]) == wit + 1 and same_bits(u, wu) and same_bits(log["resnorm"], wh)
    t = torch.from_numpy(b).cuda()
    ut, log = esp.simple(A, t, Pl=P, maxiter=7, reltol=1e-12, log=True)
    wu, wh, wit = M.simple(b, maxiter=7, reltol=1e-12)
    assert wit == 7 and same_bits(ut.cpu().numpy(), wu) and same_bits(log["resnorm"], wh)
    P.close()


# ---- update! --------------------------------------------------------------------------------------------------------------------------
def test_update_semantics(esp, model, fd):
    cp, rv, nz = (np.array(a, copy=True) for a in fd(7, 6, 5))
    A = matrix(esp, (cp, rv, nz))
    n = A.n
    lib, h = A._d.lib, A._d.h
    P = esp.AMGPreconditioner(A)
    M0 = am.AMGModel(model, (cp, rv, nz))
    v = np.random.default_rng(2).standard_normal(n)
    u0 = P.ldiv(v)
    assert same_bits(u0, M0.ldiv(v))
    # a value change in place without update!: ldiv! is unchanged (the hierarchy holds copies)
    nz2 = nz * (1.0 + 0.25 * np.random.default_rng(3).random(len(nz)))
    assert lib.esp_set_nzval(h, vp(nz2)) == 0
    assert same_bits(P.ldiv(v), u0)
    # ... and after update! it equals a fresh create
    P.update()
    M1 = am.AMGModel(model, (cp, rv, nz2))
    check_hierarchy(P, M1)
    assert same_bits(P.ldiv(v), M1.ldiv(v)) and not same_bits(M1.ldiv(v), u0)
    # a pattern change (a symmetric pair of new entries) without update!: ESP_ERR_STATE
    A.append(esp.ESP_UPDATE, [1, n], [n, 1], [-0.125, -0.25])
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.cg(A, v, Pl=P), lambda: esp.simple(A, v, Pl=P), lambda: esp.bicgstabl(A, v, Pl=P)):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    arrays = tuple(np.array(a, copy=True) for a in A.sparse().arrays())
    assert len(arrays[1]) == len(rv) + 2
    M2 = am.AMGModel(model, arrays)
    check_hierarchy(P, M2)
    assert same_bits(P.ldiv(v), M2.ldiv(v))
    Q = esp.AMGPreconditioner(A)
    check_hierarchy(Q, M2)
    Q.close()
    P.close()


# ---- the error table -----------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, args=(-1, -1, -1, -1, -1.0)):
    p = C.c_void_p()
    rc = lib.esp_precon_amg_create(h, *args, C.byref(p))
    msg = lib.esp_last_error(h)
    return rc, p, (msg.decode() if msg else "")


def test_errors(esp, fd):
    A = matrix(esp, fd(4, 3, 2))
    lib, h = A._d.lib, A._d.h
    n = A.n
    for args in ((0, -1, -1, -1, -1.0), (-2, -1, -1, -1, -1.0), (-1, 0, -1, -1, -1.0), (-1, 513, -1, -1, -1.0), (-1, -1, 0, -1, -1.0),
                 (-1, -1, -1, -2, -1.0), (-1, -1, -1, -1, float("inf")), (-1, -1, -1, -1, float("nan"))):
        rc, p, _ = raw_create(lib, h, args)
        assert rc == ESP_ERR_INVALID and not p.value, args
    rc, p, _ = raw_create(lib, h, (1, 512, 1, 0, 0.0))
    assert rc == 0 and lib.esp_precon_destroy(p) == 0
    with pytest.raises(ValueError):
        esp.AMGPreconditioner(A, presweeps=0)
    with pytest.raises(ValueError):
        esp.AMGPreconditioner(A, theta=-1.0)
    # esp_destroy of the handle is refused while the preconditioner lives
    rc, p, _ = raw_create(lib, h)
    assert rc == 0 and lib.esp_destroy(h) == ESP_ERR_STATE
    # pending entries (appended through the C call, which does not flush)
    one, val = np.ones(1, np.int64), np.ones(1)
    assert lib.esp_append_host(h, vp(one), vp(one), vp(val), None, esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h)[0] == ESP_ERR_STATE
    assert lib.esp_precon_update(p) == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    assert lib.esp_precon_update(p) == 0 and lib.esp_precon_destroy(p) == 0
    # AMG is no inner kind of a BlockPreconditioner, and esp_precon_create does not make one
    ptr, idx = np.array([0, n], np.int64), np.arange(n, dtype=np.int64)
    q = C.c_void_p()
    assert lib.esp_precon_block_create(h, esp.ESP_PRECON_AMG, 1, vp(ptr), vp(idx), 0, C.byref(q)) == ESP_ERR_INVALID
    assert lib.esp_precon_create(h, esp.ESP_PRECON_AMG, C.byref(q)) == ESP_ERR_INVALID
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, n + 1)], esp.AMGPreconditioner)
    # a rectangular matrix
    R = esp.ExtendableSparseMatrix(4, 5)
    assert raw_create(R._d.lib, R._d.h)[0] == ESP_ERR_INVALID
    # a structurally non-symmetric pattern: (1,3) is stored in column 3, (3,1) is not -- and in column 5 again
    S = sp.lil_matrix(sp.identity(6) * 2.0)
    S[1, 0] = S[0, 1] = -1.0
    S[0, 2] = -1.0
    S[3, 4] = -1.0
    U = matrix(esp, am.csc_of_scipy(S))
    rc, p, msg = raw_create(U._d.lib, U._d.h)
    assert rc == ESP_ERR_UNSUPPORTED and "column 3" in msg and "symmetric" in msg and not p.value
    # a column without a stored diagonal: the smallest one is named (and wins over the missing mirror)
    S = sp.lil_matrix(sp.identity(6) * 2.0)
    S[2, 2] = 0.0
    S[4, 4] = 0.0
    S[2, 3] = S[3, 2] = -1.0
    S[0, 5] = -1.0
    T = sp.csc_matrix(S)
    T.eliminate_zeros()
    U = matrix(esp, am.csc_of_scipy(T))
    rc, p, msg = raw_create(U._d.lib, U._d.h)
    assert rc == ESP_ERR_INVALID and "column 3" in msg and "diagonal" in msg
    # a stored zero diagonal is no error
    U = matrix(esp, full_csc(np.array([[0.0, 1.0], [1.0, 2.0]])))
    rc, p, _ = raw_create(U._d.lib, U._d.h)
    assert rc == 0 and U._d.lib.esp_precon_destroy(p) == 0
    # A still works after the failed creates
    x = np.random.default_rng(1).standard_normal(n)
    cp, rv, nz = A.sparse().arrays()
    np.testing.assert_allclose(A.mul(x), sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)) @ x, rtol=1e-13)


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.AMGPreconditioner(A)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                                       # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, vp(one), vp(one), vp(val), None, esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    rc, _, msg = raw_create(lib, h)
    assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, vp(v), vp(v), 0) == ESP_ERR_STATE
    P.close()


def test_destroy_then_create_does_not_leak(esp, fd):
    """the handle keeps no accounting of its own: the device's free memory, read through the runtime, must not keep falling"""
    import torch
    A = matrix(esp, fd(20, 20, 20))

    def cycle(k):
        for _ in range(k):
            P = esp.AMGPreconditioner(A)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(6)
    assert free0 - free1 < (8 << 20), (free0, free1)      # one hierarchy of 20^3 alone holds several MiB


# ---- the reference's acceptance test, and usefulness ----------------------------------------------------------------------------------
def test_reference_acceptance_simple_20_cubed(esp, fd):
    """test/test_preconditioners.jl:10-20,41: fdrand 20 x 20 x 20, b = ones, simple with Pl = AMG, maxiter 10000, reltol 1e-10: the
    residual norms fall over the tail, and the solution is within 1e-5 of a sparse direct solve"""
    csc = fd(20, 20, 20)
    cp, rv, nz = csc
    A = matrix(esp, csc)
    n = A.n
    b = np.ones(n)
    exact = spl.spsolve(sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)), b)
    P = esp.AMGPreconditioner(A)
    u, log = esp.simple(A, b, Pl=P, maxiter=10000, reltol=1e-10, log=True)
    h = log["resnorm"]
    nlast = min(100, len(h) // 2)
    tail = h[-nlast:]
    print("steps", len(h) - 1, "max tail ratio", (tail[1:] / tail[:-1]).max(), "error", np.linalg.norm(u - exact))
    assert np.all(tail[1:] / tail[:-1] < 1.0)
    assert np.linalg.norm(u - exact) <= 1e-5
    P.close()


def test_cg_with_amg_needs_at_most_half_of_jacobis_iterations(esp, fd):
    A = matrix(esp, fd(20, 20, 20))
    b = np.ones(A.n)
    P, J = esp.AMGPreconditioner(A), esp.JacobiPreconditioner(A)
    _, la = esp.cg(A, b, Pl=P, reltol=1e-8, log=True)
    _, lj = esp.cg(A, b, Pl=J, reltol=1e-8, log=True)
    print("cg iterations: AMG", la["iters"], "Jacobi", lj["iters"])
    assert la["isconverged"] and lj["isconverged"] and 2 * la["iters"] <= lj["iters"]
    P.close()
    J.close()
