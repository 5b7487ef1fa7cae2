"""GPU: LUFactorization on the device CSC (include/esparse_hip.h, esp_precon_lu_create) against tests/lu_model.c, bit for bit: the
permutation, the tree, the filled matrix B (colptr, rowval, nzval), the factor, the level counts and ldiv! on host vectors, device
vectors and in place; update!, the solvers, the reference's acceptance tests through A.solve / lu / lu_ / solve, the error codes."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
import lu_modellib as L
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from iluam_modellib import level_schedules
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return L.Model(tmp_path_factory.mktemp("lu_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("lu_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("lu_gmres_model"))


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


def check_order(P, want):
    """the permutation, the tree, B and the counts the model's"""
    assert np.array_equal(P.permutation(), want.c + 1)
    level, root = P.tree()
    assert level.dtype == np.int32 and np.array_equal(level, want.level) and np.array_equal(root, want.node_root + 1)
    cp, rv, nz = P.fill_matrix()
    wcp, wrv, wnz = want.B
    assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv)
    assert np.array_equal(bits(nz), bits(wnz))
    st = P.stats()
    for k in ("nnz", "rounds", "deepest", "nodes", "largest_node"):
        assert st[k] == want.stats[k], (k, st, want.stats)


def check_numeric(P, want, seed=1):
    import torch
    n = want.n
    assert same_bits(P.factor(), want.fval)
    if n:
        assert P.levels() == tuple(int(l.max()) + 1 for l in level_schedules(want.B[0], want.B[1]))
    v = np.random.default_rng(seed).standard_normal(n)
    u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u) and same_bits(P.solve(v), u)
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    t2 = torch.from_numpy(v.copy()).cuda()
    assert same_bits(P.ldiv(t2).cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


def check_all(esp, model, A, leaf_size=32, max_depth=48):
    want = model.lu(host_arrays(A), leaf_size, max_depth)
    P = esp.LUFactorization(A, leaf_size, max_depth)
    try:
        check_order(P, want)
        check_numeric(P, want)
        c, level = esp.nested_dissection(A, leaf_size, max_depth)
        assert np.array_equal(c, want.c + 1) and np.array_equal(level, want.level)
        return P.stats(), want
    finally:
        P.close()


# ---- the ordering, the tree and the fill at their edges ------------------------------------------------------------------------------
def test_empty_one_and_diagonal(esp, model):
    """n = 0, n = 1, a diagonal matrix: empty launches, all-singleton components, one round"""
    E = esp.ExtendableSparseMatrix(0, 0)
    P = esp.LUFactorization(E)
    assert P.stats()["nnz"] == 0 and len(P.permutation()) == 0 and len(P.ldiv(np.empty(0))) == 0
    P.close()
    st, _ = check_all(esp, model, from_scipy(esp, sp.csc_matrix(np.array([[4.0]]))))
    assert (st["nnz"], st["rounds"]) == (1, 1)
    st, _ = check_all(esp, model, from_scipy(esp, sp.diags(np.arange(1.0, 501.0))))
    assert (st["nnz"], st["rounds"], st["nodes"]) == (500, 1, 500)


def test_path(esp, model):
    """a path of 100 with leaf_size 8: a large eccentricity, one-vertex separators, a deep tree"""
    st, want = check_all(esp, model, from_scipy(esp, L.path(100)), 8)
    assert st["deepest"] >= 4 and st["largest_node"] <= 8


def test_arrow_gets_no_fill(esp, model):
    """ecc = 2: the hub is the separator, every spoke a leaf"""
    A = from_scipy(esp, L.arrow(200))
    st, _ = check_all(esp, model, A)
    assert st["nnz"] == A.nnz() and st["rounds"] == 2


@pytest.mark.parametrize("entries", [32, 33, 64, 65, 300])
def test_star_wave_folded_hub(esp, model, entries):
    """the hub's column holds `entries` rows, stored one way only: the vertex folded by its wave on both sides of 32 and of 64, the
    spokes' edge read from the row-wise index"""
    A = from_scipy(esp, L.star(entries))
    st, _ = check_all(esp, model, A, 8)
    assert st["nnz"] == 3 * entries - 2           # the pattern made symmetric, nothing more


def test_cliques(esp, model):
    """ecc < 2: a dense leaf above leaf_size; two cliques joined by one edge split at the joint"""
    st, _ = check_all(esp, model, from_scipy(esp, L.clique(40)), 8)
    assert (st["rounds"], st["nodes"], st["largest_node"]) == (1, 1, 40)
    st, _ = check_all(esp, model, from_scipy(esp, L.two_cliques(20)), 8)
    assert st["rounds"] >= 2 and st["nnz"] < 40 * 40


def test_leaf_size_edge(esp, model):
    """components of exactly leaf_size and leaf_size + 1 vertices: the first is a leaf, the second is split"""
    A = from_scipy(esp, L.components_of([8, 9]))
    st, want = check_all(esp, model, A, 8)
    assert np.all(want.level[:8] == 0) and want.level[8:].max() == 1


def test_block_diagonal(esp, model):
    """six 7 x 5 grids and five 3-paths, leaf_size 4: many components, roots and anc per component"""
    st, _ = check_all(esp, model, from_scipy(esp, L.block_diagonal()), 4)
    assert st["nodes"] > 11


def test_nonsymmetric_pattern(esp, model):
    """seeded, n = 300, entries stored one way only: the graph read from the column and the row index"""
    S = L.random_pattern(300, False, 0.01, 7)
    assert (S != S.T).nnz > 0 and ((S != 0) != (S != 0).T).nnz > 0
    check_all(esp, model, from_scipy(esp, S))


@pytest.mark.parametrize("name", ["fd10x10x10", "fd20x20x1", "fd17x17x17", "convdiff"])
def test_workload_shapes(esp, model, name):
    if name == "convdiff":
        check_all(esp, model, convdiff(esp, 12, 10, 8, 4.0))
        return
    dims, leaf = {"fd10x10x10": ((10, 10, 10), 16), "fd20x20x1": ((20, 20, 1), 8), "fd17x17x17": ((17, 17, 17), 32)}[name]
    st, _ = check_all(esp, model, esp.fdrand(*dims), leaf)
    if name == "fd10x10x10":
        assert (st["rounds"], st["deepest"], st["nnz"]) == (8, 7, 78308)


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_depth_cap(esp, model, max_depth):
    """the depth cap: what is left becomes dense leaves (max_depth = 0: one dense leaf of 1000 columns, the slowest matrix for
    ILUAM's column chains -- the order, B, the factor and one ldiv! are compared; the other forms of ldiv! have their cases above)"""
    A = esp.fdrand(10, 10, 10)
    want = model.lu(host_arrays(A), 16, max_depth)
    P = esp.LUFactorization(A, 16, max_depth)
    check_order(P, want)
    assert same_bits(P.factor(), want.fval)
    v = np.random.default_rng(1).standard_normal(A.n)
    assert same_bits(P.ldiv(v), want.ldiv(v))
    st = P.stats()
    P.close()
    assert st["rounds"] == max_depth + 1
    if max_depth == 0:
        assert st["nnz"] == 1000 * 1000


def struct_lengths(F):
    bcp, brv, _ = F.B
    return [int((brv[bcp[s] - 1:bcp[s + 1] - 1] - 1 >= s + F.nsize[s]).sum()) for s in np.unique(F.nstart)]


@pytest.mark.parametrize("rows,nx,ny", [(63, 61, 64), (64, 47, 94), (65, 63, 66)])
def test_struct_lists_at_the_wave_edge(esp, model, rows, nx, ny):
    """2-D grids with leaf_size 4 whose longest struct list holds 63 / 64 / 65 rows (found with the model): the lanes of the
    expansion kernel stride the list 64 at a time"""
    A = from_scipy(esp, L.dominant(L.edges_pattern(nx * ny, L.grid_edges(nx, ny))))
    st, want = check_all(esp, model, A, 4)
    assert max(struct_lengths(want)) == rows


def test_stored_zeros_and_nan(esp, model):
    """stored 0.0, -0.0 and NaN off-diagonals in a 5 x 4 x 3 grid: the graph is the pattern alone, the values move bitwise"""
    cp, rv, nz = host_arrays(esp.fdrand(5, 4, 3))
    off = [q for j in range(len(cp) - 1) for q in range(cp[j] - 1, cp[j + 1] - 1) if rv[q] != j + 1]
    nz[off[3]], nz[off[10]], nz[off[17]] = 0.0, -0.0, np.nan
    A = from_arrays(esp, cp, rv, nz)
    want = model.lu((cp, rv, nz))
    ref = model.lu(host_arrays(esp.fdrand(5, 4, 3)))
    assert np.array_equal(want.c, ref.c) and np.array_equal(want.B[1], ref.B[1])
    P = esp.LUFactorization(A)
    check_order(P, want)
    check_numeric(P, want)
    assert np.signbit(P.fill_matrix()[2]).sum() == np.signbit(want.B[2]).sum() and np.isnan(P.fill_matrix()[2]).sum() == 1
    P.close()


# ---- updates -------------------------------------------------------------------------------------------------------------------------
def test_values_only_update_equals_fresh_create(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.LUFactorization(A, 8)
    launches = P.stats()["launches"]
    assert launches > 0
    v = np.random.default_rng(6).standard_normal(n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: the values of the last update!
    P.update()
    assert P.stats()["launches"] == launches              # the ordering was not run again
    want = model.lu(host_arrays(A), 8)
    F = esp.LUFactorization(A, 8)
    for Q in (P, F):
        check_order(Q, want)
    u_new = check_numeric(P, want, seed=6)
    assert same_bits(F.ldiv(v), u_new) and not same_bits(u_new, u_old)
    assert same_bits(P.factor(), F.factor())
    F.close()
    P.close()


def test_pattern_change_needs_update_and_rebuilds(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.LUFactorization(A, 8)
    launches = P.stats()["launches"]
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.25])       # two corners
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.gmres(A, v, Pl=P), P.permutation, P.tree):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    assert P.stats()["launches"] > launches                # everything anew
    want = model.lu(host_arrays(A), 8)
    check_order(P, want)
    u = check_numeric(P, want, seed=6)
    F = esp.LUFactorization(A, 8)
    assert same_bits(F.ldiv(v), u)
    F.close()
    P.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, leaf=32, depth=48):
    p = C.c_void_p()
    rc = lib.esp_precon_lu_create(h, leaf, depth, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for leaf, depth in ((0, 48), (-3, 48), (32, -1), (32, 65)):
        assert raw_create(lib, h, leaf, depth)[0] == ESP_ERR_INVALID
        assert lib.esp_nested_dissection(h, leaf, depth, None, None, 0) == ESP_ERR_INVALID
    p = C.c_void_p()
    assert lib.esp_precon_lu_create(None, 32, 48, C.byref(p)) == ESP_ERR_INVALID and lib.esp_precon_lu_create(h, 32, 48, None) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h)[0] == ESP_ERR_INVALID
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))   # no stored (3,3)
    rc, _, msg = raw_create(M._d.lib, M._d.h)
    assert rc == ESP_ERR_INVALID and "diagonal" in msg and "A's column is 3" in msg
    one, val = np.ones(1, np.int64), np.ones(1)                                              # pending entries
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # the other kinds' accessors refuse an LU factorization and the other way round
    rc, p, _ = raw_create(lib, h)
    assert rc == 0
    b, path = C.c_void_p(), C.c_int32()
    assert lib.esp_precon_block_matrix(p, C.byref(b), C.byref(path)) == ESP_ERR_INVALID
    assert lib.esp_precon_colored_matrix(p, C.byref(b)) == ESP_ERR_INVALID and lib.esp_precon_iluk_matrix(p, C.byref(b)) == ESP_ERR_INVALID
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 2, C.byref(q)) == 0
    out = (C.c_int64 * 6)()
    assert lib.esp_precon_lu_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_lu_matrix(q, C.byref(b)) == ESP_ERR_INVALID
    assert lib.esp_precon_lu_perm(q, out, 0) == ESP_ERR_INVALID and lib.esp_precon_lu_tree(q, None, None, 0) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(q) == 0
    # the handle refuses destroy while the factorization lives
    assert lib.esp_destroy(h) == ESP_ERR_STATE
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_fill_guard_refuses_before_b_is_allocated(esp, model):
    """the 2^32 - 16 guard on nnz(B), reached through esp_debug_lu_fill_cap: ESP_ERR_UNSUPPORTED with nnz(B) in the message; a
    refused update! after a pattern change leaves the earlier factorization usable"""
    A = esp.fdrand(5, 4, 3)
    lib, h = A._d.lib, A._d.h
    want = model.lu(host_arrays(A))
    assert lib.esp_debug_lu_fill_cap(h, -1) == ESP_ERR_INVALID
    assert lib.esp_debug_lu_fill_cap(h, want.stats["nnz"]) == 0
    rc, _, msg = raw_create(lib, h)
    assert rc == ESP_ERR_UNSUPPORTED and str(want.stats["nnz"]) in msg
    assert lib.esp_debug_lu_fill_cap(h, want.stats["nnz"] + 1) == 0
    Q = esp.LUFactorization(A)                               # one below the cap: accepted
    Q.close()
    assert lib.esp_debug_lu_fill_cap(h, 0) == 0
    P = esp.LUFactorization(A)
    launches = P.stats()["launches"]
    A.append(esp.ESP_UPDATE, [A.n, 1], [1, A.n], [0.5, 0.25])
    A.flush()
    want2 = model.lu(host_arrays(A))
    assert lib.esp_debug_lu_fill_cap(h, want2.stats["nnz"]) == 0
    with pytest.raises(esp.EspError) as e:
        P.update()                                           # refused before B is replaced
    assert e.value.code == ESP_ERR_UNSUPPORTED and str(want2.stats["nnz"]) in str(e.value)
    st = P.stats()
    assert st["nnz"] == want.stats["nnz"] and st["launches"] == launches      # the earlier state
    cp, rv, nz = P.fill_matrix()
    assert np.array_equal(rv, want.B[1]) and np.array_equal(bits(nz), bits(want.B[2]))
    assert lib.esp_debug_lu_fill_cap(h, 0) == 0
    P.update()
    check_order(P, want2)
    check_numeric(P, want2)
    P.close()


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.LUFactorization(A)
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
    assert lib.esp_nested_dissection(h, 32, 48, None, None, 0) == ESP_ERR_UNSUPPORTED
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, v.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_STATE
    P.close()


def test_create_destroy_loop_does_not_leak(esp):
    """the device's free memory, read through the runtime, must not keep falling over 20 create / update / destroy cycles"""
    import torch
    A = esp.fdrand(8, 7, 6)

    def cycle(k):
        for _ in range(k):
            P = esp.LUFactorization(A, 8)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(20)
    assert free0 - free1 < (8 << 20), (free0, free1)


# ---- solvers ---------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! driven with the LU model's ldiv and A's mul"""

    def __init__(self, lib, fact):
        self.m, self.P, self.csc, self.n = lib, fact, fact.csc, fact.n

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
    P = esp.LUFactorization(A, 8)
    M = SolverModel(solver_lib, model.lu(arrays, 8))
    x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True)
    wx, wh, wit, wconv = M.cg(b)
    assert log["iters"] == wit and log["isconverged"] == wconv and wconv
    assert same_bits(history_of(log), wh) and same_bits(x if where == "host" else x.cpu().numpy(), wx)
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_nonsymmetric_solvers(esp, model, solver_lib, gmres_lib, where):
    """bicgstabl(l = 2), gmres(restart = 20) and simple! (iterative refinement) on the convection-diffusion matrix: the iteration
    counts, histories and solutions of the solver models over the model's ldiv"""
    A = convdiff(esp, 6, 5, 4, 2.0)
    n = A.n
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.LUFactorization(A, 8)
    M = SolverModel(solver_lib, model.lu(arrays, 8))
    x, log = esp.bicgstabl(A, dev(b), l=2, Pl=P, log=True)
    wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2)
    # (an exact Pl leaves BiCGStab(l) nothing to minimise after its first step: the model's own outcome is asserted, whatever it is)
    assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv)
    assert same_bits(history_of(log), wh) and same_bits(host(x), wx)
    print("bicgstabl(l = 2) with Pl = LUFactorization: iters %d, mvps %d, converged %s, history %s" % (wit, wmv, wconv, wh[:4]))
    x, log = esp.gmres(A, dev(b), Pl=P, restart=20, log=True)
    want = gmres_lib.gmres_cb(M, n, b, restart=20)
    assert (log["iters"], log["mvps"], log["reorth"], log["isconverged"]) == (want.iters, want.mvps, want.reorth, want.converged)
    assert want.converged and same_bits(history_of(log), want.history) and same_bits(host(x), want.x)
    u0 = np.random.default_rng(12).standard_normal(n)
    got, log = esp.simple(A, dev(b), u=dev(u0.copy()), Pl=P, maxiter=3, reltol=0.0, log=True)
    wu, wh, wit = M.simple(b, u=u0, maxiter=3, reltol=0.0)
    assert wit == 3 and same_bits(host(got), wu) and same_bits(log["resnorm"], wh)
    got, log = esp.simple(A, dev(b), Pl=P, log=True)                       # to its default tolerance: the model's step count
    wu, wh, wit = M.simple(b)
    assert len(log["resnorm"]) == len(wh) and same_bits(host(got), wu)
    P.close()


# ---- the reference's acceptance tests on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(100, 1, 1), (20, 20, 1), (10, 10, 10)])
def test_reference_backslash(esp, grid):
    """test/test_backslash.jl through A.solve(b) and solve(A, b), host and device vectors"""
    A = esp.fdrand(*grid, rand_mode=0)
    x = np.ones(A.n)
    b = A.mul(x)
    got = A.solve(b)
    assert np.linalg.norm(got - x) <= 10.0 * np.sqrt(EPS)
    assert same_bits(esp.solve(A, b), got) and same_bits(A.solve(to_device(b)).cpu().numpy(), got)


def add_to_diagonal(esp, A, by):
    d = np.arange(1, A.n + 1)
    A.append(esp.ESP_UPDATE, d, d, np.full(A.n, by))
    A.flush()


@pytest.mark.parametrize("grid", [(10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu1(esp, grid):
    """test/test_lu.jl:7-31 through lu / lu_ / update: both answers agree with a dense solve to 100 sqrt(eps), relative"""
    A = esp.fdrand(*grid, rand_mode=0)
    b = np.random.default_rng(11).random(A.n)
    F = esp.lu(A)
    assert esp.issolver(F) and esp.lu_(F, A) is F
    x1 = F.solve(b)
    a1 = sp.csc_matrix((host_arrays(A)[2], host_arrays(A)[1] - 1, host_arrays(A)[0] - 1), shape=(A.n, A.n)).toarray()
    add_to_diagonal(esp, A, 1.0)
    launches = F.stats()["launches"]
    assert esp.factorize_(F, A) is F and F.stats()["launches"] == launches
    x2 = F.solve(b)
    a2 = a1 + np.eye(A.n)
    for x, a in ((x1, a1), (x2, a2)):
        ref = np.linalg.solve(a, b)
        assert np.linalg.norm(ref - x) / np.linalg.norm(ref) <= 100.0 * np.sqrt(EPS)
    assert same_bits(A.solve(b), x2)
    F.close()


@pytest.mark.parametrize("grid", [(10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu2(esp, grid):
    """test/test_lu.jl:33-45: after A[i,i+3] -= 1e-4, A[i-3,i] -= 1e-4 (a pattern change) and lu_, every component of the new
    solution exceeds the old one; lu_ with another matrix binds the factorization anew"""
    A = esp.fdrand(*grid, rand_mode=0)
    n = A.n
    b = np.random.default_rng(12).random(n)
    F = esp.lu(A)
    x1 = F.solve(b)
    i = np.arange(4, n - 3 + 1)
    A.append(esp.ESP_UPDATE, np.concatenate([i, i - 3]), np.concatenate([i + 3, i]), np.full(2 * len(i), -1.0e-4))
    A.flush()
    nnz_b = F.stats()["nnz"]
    assert esp.lu_(F, A) is F and F.stats()["nnz"] > nnz_b
    x2 = F.solve(b)
    assert np.all(x1 < x2)
    B = esp.fdrand(*grid, rand_mode=0)
    assert esp.lu_(F, B) is F and F.A is B and same_bits(F.solve(b), x1)
    F.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    for kw in ({"leaf_size": 0}, {"leaf_size": 1.5}, {"max_depth": -1}, {"max_depth": 65}):
        with pytest.raises(ValueError):
            esp.LUFactorization(A, **kw)
    P = esp.SparspakLU(A)
    assert isinstance(P, esp.LUFactorization) and esp.issolver(P) and not esp.issolver(esp.ILU0Preconditioner(A))
    assert (P.leaf_size, P.max_depth) == (32, 48) and isinstance(P.stats(), dict)
    b = A.mul(np.ones(A.n))
    assert np.linalg.norm(P.solve(b) - 1.0) <= 1e-12 * np.sqrt(A.n)
    for solve in (esp.cg, esp.gmres, esp.bicgstabl, esp.simple):
        assert np.linalg.norm(solve(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    with pytest.raises(TypeError) as e:
        esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.LUFactorization)          # no inner kind of the block preconditioner
    assert "LUFactorization" in str(e.value)
    with pytest.raises(TypeError):
        esp.ColoredPreconditioner(A, esp.LUFactorization)
    c, level = esp.nested_dissection(A)
    assert np.array_equal(c, P.permutation()) and np.array_equal(level, P.tree()[0])
    P.close()
    with pytest.raises(ValueError):
        P.solve(b)
