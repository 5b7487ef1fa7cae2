"""GPU: RS_AMGPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_rsamg_create) against the model of
tests/rsamg_modellib.py (rsamg_model.c is normative): the splitting and its rounds on every level, every P_l and A_l, rho_l, the
coarsest level's inverse, ldiv! and x with the whole residual history of cg, bicgstabl, gmres and simple! bit for bit (a NaN equals
a NaN at the same position: its payload is not pinned); update!, the error table and leaks as for AMGPreconditioner; and that the
preconditioner is worth having: half of Jacobi's iterations at the most."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_modellib as am
import rsamg_modellib as rs
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_NOMEM, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -4, -5, -6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return rs.Model(tmp_path_factory.mktemp("rsamg_model"))


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
    return rs.graphs(fd)


@pytest.fixture(scope="module")
def m20(model, fd):
    """the model hierarchy of fdrand 20 x 20 x 20 with the defaults: computed once, shared, left unchanged"""
    return rs.RSAMGModel(model, fd(20, 20, 20))


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
    assert P.coarsening == 1 and P.levels == len(M.levels)
    for l, L in enumerate(M.levels):
        D = P.level(l)
        assert D["n"] == L.n and D["rounds"] == L.rounds, (l, D["n"], L.n, D["rounds"], L.rounds)
        assert same_bits([D["rho"]], [L.rho]), (l, D["rho"], L.rho)
        for got, want in ((D["A"], L.A), (D["P"], L.P)):
            assert (got is None) == (want is None), l
            if want is not None:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), l
                assert same_bits(got[2], want[2]), l
        if L.cf is not None:
            cf = P.splitting(l)
            assert np.array_equal(cf, L.cf), l
            assert int(np.sum(cf >= 0)) == L.nc
            if L.P is not None:
                assert M.levels[l + 1].n == L.nc
        else:
            with pytest.raises(Exception):
                P.splitting(l)
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


def check_all(esp, model, csc, M=None, **kw):
    A = matrix(esp, csc)
    P = esp.RS_AMGPreconditioner(A, **kw)
    try:
        if M is None:
            with np.errstate(all="ignore"):
                M = rs.RSAMGModel(model, csc, **kw)
        check_hierarchy(P, M)
        check_ldiv(P, M)
        return M
    finally:
        P.close()


# ---- the splitting, its rounds and the whole hierarchy on the graphs of the issue ---------------------------------------------------
@pytest.mark.parametrize("name,theta", rs.GRAPH_CASES)
def test_splitting_and_hierarchy(esp, model, graphs, name, theta):
    """max_coarse = 1: every level with more than one unknown is split.  n = 0, 1, 2; star33 .. star130: a row and a column on
    either side of the 32-entry and 64-entry whole-wave limits; dirichlet: rows with an empty S_i; dense70: rows longer than a
    wave; convection-diffusion at Pe 4 and Pe 50: one-directional strength; posmix: positive couplings"""
    csc = graphs[name]
    M = check_all(esp, model, csc, max_coarse=1, theta=theta)
    n = len(csc[0]) - 1
    if n > 1:
        assert M.levels[0].cf is not None and M.levels[0].rounds >= 1 and M.levels[-1].n == 1
    if name.startswith("star"):
        assert np.diff(csc[0]).max() == n and [L.n for L in M.levels] == [n, 1]        # the hub's column: the whole-wave path
    if name == "dirichlet":
        assert int(np.sum(M.levels[0].cf == -2)) >= 7
    if name == "posmix":
        without, with_c = rs.positive_branches(model, csc, theta)
        assert without >= 1 and with_c >= 1


def test_default_parameters_through_the_raw_abi(esp, model, fd):
    csc = fd(5, 5, 5)
    A = matrix(esp, csc)
    lib, h = A._d.lib, A._d.h
    p = C.c_void_p()
    assert lib.esp_precon_rsamg_create(h, -1, -1, -1, -1, -1.0, C.byref(p)) == 0    # -1 / a negative theta: 10, 64, 1, 1, 0.25
    M = rs.RSAMGModel(model, csc)
    assert len(M.levels) >= 2
    v = np.random.default_rng(3).standard_normal(A.n)
    u = np.empty_like(v)
    assert lib.esp_precon_ldiv(p, vp(v), vp(u), 0) == 0 and same_bits(u, M.ldiv(v))
    kind = C.c_int32(7)
    assert lib.esp_precon_amg_coarsening(p, C.byref(kind)) == 0 and kind.value == esp.ESP_AMG_COARSEN_RS == 1
    cf = np.full(A.n, -7, np.int64)
    assert lib.esp_precon_amg_splitting(p, 0, vp(cf), 0) == 0 and np.array_equal(cf, M.levels[0].cf)
    out = (C.c_int64 * 3)(7, 7, 7)
    assert lib.esp_precon_levels(p, out) == 0 and list(out) == [0, 0, 0]
    assert lib.esp_precon_get_factor(p, vp(u), 0) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(p) == 0
    # theta = 0.25 is not the same hierarchy as theta = 0: the default is really 0.25
    assert [L.n for L in rs.RSAMGModel(model, csc, theta=0.0).levels] != [L.n for L in M.levels]
    P = esp.RS_AMGPreconditioner(A)
    check_hierarchy(P, M)
    P.close()


def test_inspection_into_device_memory_and_the_other_coarsening(esp, model, fd):
    import torch
    csc = fd(7, 6, 5)
    A = matrix(esp, csc)
    P = esp.RS_AMGPreconditioner(A)
    M = rs.RSAMGModel(model, csc)
    lib = A._d.lib
    cf = torch.full((A.n,), -7, dtype=torch.int64, device="cuda")
    nl = M.levels[-1].n
    inv = torch.zeros(nl * nl, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert lib.esp_precon_amg_splitting(P._p, 0, C.c_void_p(cf.data_ptr()), 1) == 0
    assert lib.esp_precon_amg_coarse_inverse(P._p, C.c_void_p(inv.data_ptr()), 1) == 0
    assert np.array_equal(cf.cpu().numpy(), M.levels[0].cf) and same_bits(inv.cpu().numpy().reshape(nl, nl), M.inv)
    assert lib.esp_precon_amg_splitting(P._p, P.levels - 1, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID     # not split
    assert lib.esp_precon_amg_splitting(P._p, P.levels, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID         # no such level
    assert lib.esp_precon_amg_splitting(P._p, -1, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID
    # each inspector refuses the other coarsening
    assert lib.esp_precon_amg_aggregates(P._p, 0, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID
    Q = esp.AMGPreconditioner(A)
    assert Q.coarsening == esp.ESP_AMG_COARSEN_SA == 0 and P.coarsening == 1
    assert lib.esp_precon_amg_splitting(Q._p, 0, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID
    assert lib.esp_precon_amg_aggregates(Q._p, 0, C.c_void_p(cf.data_ptr()), 1) == 0
    assert not hasattr(Q, "splitting")
    kind = C.c_int32()
    assert lib.esp_precon_amg_coarsening(None, C.byref(kind)) == ESP_ERR_INVALID
    assert lib.esp_precon_amg_coarsening(P._p, None) == ESP_ERR_INVALID
    J = esp.JacobiPreconditioner(A)
    assert lib.esp_precon_amg_coarsening(J._p, C.byref(kind)) == ESP_ERR_INVALID
    assert lib.esp_precon_amg_splitting(J._p, 0, C.c_void_p(cf.data_ptr()), 1) == ESP_ERR_INVALID
    for X in (P, Q, J):
        X.close()


def test_hierarchy_keeps_an_explicit_zero_a_negative_zero_and_a_nan(esp, model, fd):
    cp, rv, nz = (np.array(a, copy=True) for a in fd(6, 5, 4))

    def pos(i, j):
        k = cp[j] - 1 + np.searchsorted(rv[cp[j] - 1:cp[j + 1] - 1], i + 1)
        assert rv[k] == i + 1
        return k
    nz[pos(0, 1)] = nz[pos(1, 0)] = 0.0          # a stored zero pair: no dependence
    nz[pos(7, 13)] = -0.0                        # one side -0.0: 13 still depends on 7
    nz[pos(50, 56)] = np.nan                     # a NaN: never strong, and it spreads through the Galerkin products
    check_all(esp, model, (cp, rv, nz), max_coarse=8)


# ---- ldiv! ----------------------------------------------------------------------------------------------------------------------------
def test_ldiv_5x5x5(esp, model, fd):
    M = check_all(esp, model, fd(5, 5, 5))
    assert len(M.levels) == 2


def test_ldiv_20_cubed_defaults(esp, model, fd, m20):
    check_all(esp, model, fd(20, 20, 20), M=m20)
    assert len(m20.levels) >= 4 and m20.inv is not None


@pytest.mark.parametrize("sweeps", [(2, 2), (1, 0), (3, 1)])
def test_ldiv_sweeps(esp, model, fd, sweeps):
    check_all(esp, model, fd(20, 20, 20), presweeps=sweeps[0], postsweeps=sweeps[1])


@pytest.mark.parametrize("max_levels", [1, 2, 10])
def test_ldiv_max_levels(esp, model, fd, max_levels):
    """max_levels = 1 and 2 end at 8000 and at the first coarse level, both above 512 unknowns: the coarsest level is only smoothed"""
    M = check_all(esp, model, fd(20, 20, 20), max_levels=max_levels)
    assert len(M.levels) == min(max_levels, 5)
    assert (M.inv is None) == (max_levels < 3) and (M.levels[-1].n > 512) == (max_levels < 3)


def test_smoothing_only_coarsest_where_the_splitting_stalls(esp, model):
    """max_coarse is at most 512, so a coarsest level above it comes from max_levels (above) or from a splitting that leaves no C
    point: a diagonal matrix of 600 unknowns, every S_i empty, no round"""
    n = 600
    csc = (np.arange(1, n + 2, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64), 1.0 + np.arange(n) / n)
    M = check_all(esp, model, csc, max_coarse=512)
    assert len(M.levels) == 1 and M.inv is None and M.levels[0].nc == 0 and M.levels[0].rounds == 0
    assert np.all(M.levels[0].cf == -2)


# ---- the solvers with Pl = RS: x and the whole residual history -------------------------------------------------------------------
def test_cg_with_rs(esp, model, fd):
    import torch
    csc = fd(12, 12, 12)
    A = matrix(esp, csc)
    P = esp.RS_AMGPreconditioner(A)
    M = rs.RSAMGModel(model, csc)
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


def test_bicgstabl_and_gmres_with_rs_on_convection_diffusion(esp, model, tmp_path_factory):
    import gmres_modellib
    csc = am.convdiff(6, 5, 4, 4.0)
    A = matrix(esp, csc)
    P = esp.RS_AMGPreconditioner(A)
    M = rs.RSAMGModel(model, csc)
    check_hierarchy(P, M)
    b = np.random.default_rng(9).standard_normal(A.n)
    wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2, reltol=1e-8)
    x, log = esp.bicgstabl(A, b, l=2, Pl=P, reltol=1e-8, log=True)
    assert log["iters"] == wit and log["mvps"] == wmv and log["isconverged"] == wconv and wconv
    assert same_bits(x, wx) and same_bits(np.concatenate([[log["r0"]], log["resnorm"]]), wh)
    gm = gmres_modellib.Model(tmp_path_factory.mktemp("gmres_model"))
    want = gm.gmres_cb(M, A.n, b, restart=20)
    x, log = esp.gmres(A, b, Pl=P, restart=20, log=True)
    assert log["iters"] == want.iters and log["mvps"] == want.mvps and log["reorth"] == want.reorth
    assert log["isconverged"] == want.converged and want.converged and want.iters > 3
    assert same_bits(np.concatenate([[log["r0"]], log["resnorm"]]), want.history) and same_bits(x, want.x)
    P.close()


def test_simple_with_rs(esp, model, fd):
    import torch
    csc = fd(5, 5, 5)
    A = matrix(esp, csc)
    P = esp.RS_AMGPreconditioner(A)
    M = rs.RSAMGModel(model, csc)
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
    P = esp.RS_AMGPreconditioner(A)
    M0 = rs.RSAMGModel(model, (cp, rv, nz))
    v = np.random.default_rng(2).standard_normal(n)
    u0 = P.ldiv(v)
    assert same_bits(u0, M0.ldiv(v))
    # a value change in place without update!: ldiv! is unchanged (the hierarchy holds copies)
    nz2 = nz * (1.0 + 0.25 * np.random.default_rng(3).random(len(nz)))
    assert lib.esp_set_nzval(h, vp(nz2)) == 0
    assert same_bits(P.ldiv(v), u0)
    # ... and after update! it equals a fresh create
    P.update()
    M1 = rs.RSAMGModel(model, (cp, rv, nz2))
    check_hierarchy(P, M1)
    assert same_bits(P.ldiv(v), M1.ldiv(v)) and not same_bits(M1.ldiv(v), u0)
    # a pattern change (a symmetric pair of new entries) without update!: ESP_ERR_STATE
    A.append(esp.ESP_UPDATE, [1, n], [n, 1], [-0.125, -0.25])
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.cg(A, v, Pl=P), lambda: esp.simple(A, v, Pl=P), lambda: esp.bicgstabl(A, v, Pl=P),
                 lambda: esp.gmres(A, v, Pl=P)):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    arrays = tuple(np.array(a, copy=True) for a in A.sparse().arrays())
    assert len(arrays[1]) == len(rv) + 2
    M2 = rs.RSAMGModel(model, arrays)
    check_hierarchy(P, M2)
    assert same_bits(P.ldiv(v), M2.ldiv(v))
    Q = esp.RS_AMGPreconditioner(A)
    check_hierarchy(Q, M2)
    Q.close()
    P.close()


# ---- the error table -----------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, args=(-1, -1, -1, -1, -1.0)):
    p = C.c_void_p()
    rc = lib.esp_precon_rsamg_create(h, *args, C.byref(p))
    msg = lib.esp_last_error(h)
    return rc, p, (msg.decode() if msg else "")


def full_csc(a):
    n = a.shape[0]
    return 1 + n * np.arange(n + 1, dtype=np.int64), np.tile(np.arange(1, n + 1, dtype=np.int64), n), np.ascontiguousarray(a.T).reshape(-1)


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
    assert lib.esp_precon_rsamg_create(None, -1, -1, -1, -1, -1.0, C.byref(p)) == ESP_ERR_INVALID
    assert lib.esp_precon_rsamg_create(h, -1, -1, -1, -1, -1.0, None) == ESP_ERR_INVALID
    with pytest.raises(ValueError):
        esp.RS_AMGPreconditioner(A, presweeps=0)
    with pytest.raises(ValueError):
        esp.RS_AMGPreconditioner(A, theta=-1.0)
    with pytest.raises(TypeError):
        esp.RS_AMGPreconditioner(np.eye(3))
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
    # RS is no inner kind of a BlockPreconditioner
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, n + 1)], esp.RS_AMGPreconditioner)
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
    P = esp.RS_AMGPreconditioner(A)
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
            P = esp.RS_AMGPreconditioner(A)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(6)
    assert free0 - free1 < (8 << 20), (free0, free1)      # one hierarchy of 20^3 alone holds several MiB


# ---- usefulness ---------------------------------------------------------------------------------------------------------------------
def test_cg_with_rs_needs_at_most_half_of_jacobis_iterations(esp, fd):
    A = matrix(esp, fd(20, 20, 20))
    b = np.ones(A.n)
    P, J = esp.RS_AMGPreconditioner(A), esp.JacobiPreconditioner(A)
    _, lr = esp.cg(A, b, Pl=P, reltol=1e-8, log=True)
    _, lj = esp.cg(A, b, Pl=J, reltol=1e-8, log=True)
    print("cg iterations on fd 20^3: RS", lr["iters"], "Jacobi", lj["iters"])
    assert lr["isconverged"] and lj["isconverged"] and 2 * lr["iters"] <= lj["iters"]
    P.close()
    J.close()


def test_gmres_with_rs_needs_at_most_half_of_jacobis_iterations_on_convection_diffusion(esp):
    A = matrix(esp, am.convdiff(12, 10, 8, 4.0))
    b = np.random.default_rng(9).standard_normal(A.n)
    P, J = esp.RS_AMGPreconditioner(A), esp.JacobiPreconditioner(A)
    _, lr = esp.gmres(A, b, Pl=P, restart=20, log=True)
    _, lj = esp.gmres(A, b, Pl=J, restart=20, log=True)
    print("gmres(20) iterations on convdiff(12,10,8) at Pe 4: RS", lr["iters"], "Jacobi", lj["iters"])
    assert lr["isconverged"] and lj["isconverged"] and 2 * lr["iters"] <= lj["iters"]
    P.close()
    J.close()
