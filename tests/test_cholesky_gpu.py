"""GPU: CholeskyFactorization on the device CSC (include/esparse_hip.h, esp_precon_cholesky_create) against tests/cholesky_model.c,
bit for bit: the permutation, the tree, L (pattern and values) and ldiv! on host vectors, device vectors and in place; both forms
of the numeric factorization, update!, the launch counts, the error codes, the reference's acceptance tests, the solvers.

The tile and block dimensions T of csrc/cholesky.hip and the sizes that straddle them:
  NB = 32      columns of the update tile = the factor block width = W_small (the wide form starts at width 33)
  KB = 16      columns of a descendant (or of the node itself) staged in LDS at once
  TR = 64      rows of the update tile
  FR = 128     rows below the diagonal block one workgroup divides (rows below the first block column: width - 32)
  CT = 256     lanes of a workgroup: the rows one pass of the solves takes
  TRI_LDS = 1024  rows of a node's triangle the solves keep in LDS (a wider node uses a second vector)
Node widths T - 1, T, T + 1 are dense nodes: fdrand n x 1 x 1 with max_depth = 0 (one leaf of width n, h = 0), n in
  1, 2 | 15, 16, 17 | 31, 32, 33 | 63, 64, 65 (65: above two blocks) | 127, 128, 129 | 159, 160, 161 (128 rows below the first block)
  | 255, 256, 257 | 1023, 1024, 1025.
Separator widths at the same edges: k x k x 1 grids (the top separator is k wide and has descendants on both sides),
  k in 15, 16, 17, 31, 32, 33, 63, 64, 65.
Struct heights at the row-tile edge: the 2-D grids 61 x 64, 47 x 94, 63 x 66 with leaf_size 4, whose longest struct list holds
  63 / 64 / 65 rows (the shapes tests/test_lu_gpu.py found with the LU model; asserted here on the Cholesky model's pattern).
Update lists: length 0 (every leaf), 2 (a path of 3 with leaf_size 1; the shortest list a separator can have: both sides of a split
  touch it, so length 1 does not occur in this tree) and 199 (the arrow's hub).  A workgroup stages ONE descendant at a time, KB
  of its columns per step: every list longer than 1 and every descendant wider than 16 is "longer than what is staged at once".

The launch bound of the numeric factorization (test_launch_counts): one load launch; per depth one launch for all its small nodes
(if any) and two launches (tiles + diagonal blocks, rows below) per block column of its widest wide node:
  factor_launches <= 1 + (deepest + 1) + 2 * wide_block_columns,
wide_block_columns = the sum over the depths of ceil(width of the widest wide node / 32), which stats() reports."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import cholesky_modellib as CM
import gmres_modellib
import lu_modellib as L
from block_precon_modellib import BlockModel
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE, ESP_ERR_NOTPOSDEF = -1, -5, -6, -8
EPS = np.finfo(np.float64).eps
EVERYTHING_SMALL = 2 ** 30


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return CM.Model(tmp_path_factory.mktemp("cholesky_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("cholesky_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("cholesky_gmres_model"))


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
    n = S.shape[0]
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def from_arrays(esp, cp, rv, nz):
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(len(cp) - 1, len(cp) - 1, cp, rv, nz))


def to_device(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def check_order(P, want):
    assert np.array_equal(P.permutation(), want.c + 1)
    level, root = P.tree()
    assert level.dtype == np.int32 and np.array_equal(level, want.level) and np.array_equal(root, want.node_root + 1)
    st = P.stats()
    for k in ("nnz", "rounds", "deepest", "nodes", "largest_node"):
        assert st[k] == want.stats[k], (k, st, want.stats)


def check_numeric(P, want, seed=1):
    cp, rv, nz = P.factor()
    assert np.array_equal(cp, want.L[0]) and np.array_equal(rv, want.L[1])
    assert same_bits(nz, want.L[2])
    n = want.n
    v = np.random.default_rng(seed).standard_normal(n)
    u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u) and same_bits(P.solve(v), u)
    t = to_device(v)
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    assert same_bits(P.ldiv(to_device(v)).cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


def check_all(esp, model, A, leaf_size=32, max_depth=48, wide_from=0):
    want = model.cholesky(host_arrays(A), leaf_size, max_depth)
    assert A._d.lib.esp_debug_cholesky_wide_from(A._d.h, wide_from) == 0
    P = esp.CholeskyFactorization(A, leaf_size, max_depth)
    try:
        check_order(P, want)
        check_numeric(P, want)
        return P.stats(), want
    finally:
        P.close()
        assert A._d.lib.esp_debug_cholesky_wide_from(A._d.h, 0) == 0


# ---- matrix shapes ---------------------------------------------------------------------------------------------------------------------
def test_empty_one_and_diagonal(esp, model):
    E = esp.ExtendableSparseMatrix(0, 0)
    P = esp.CholeskyFactorization(E)
    st = P.stats()
    assert st["nnz"] == 0 and st["ldiv_launches"] == 0 and len(P.permutation()) == 0 and len(P.ldiv(np.empty(0))) == 0
    assert [len(a) for a in P.factor()] == [1, 0, 0]
    P.close()
    st, _ = check_all(esp, model, from_scipy(esp, sp.csc_matrix(np.array([[4.0]]))))
    assert (st["nnz"], st["rounds"], st["panel_doubles"]) == (1, 1, 1)
    st, _ = check_all(esp, model, from_scipy(esp, sp.diags(np.arange(1.0, 501.0))))       # 500 nodes of width 1, h = 0
    assert (st["nnz"], st["rounds"], st["nodes"], st["panel_doubles"]) == (500, 1, 500, 500)


def test_arrow(esp, model):
    """width-1 leaves with h = 1, and the hub's update list of 199 descendants"""
    A = from_scipy(esp, L.arrow(200))
    st, _ = check_all(esp, model, A)
    assert st["nnz"] == 200 + 199 and st["rounds"] == 2
    check_all(esp, model, A, wide_from=1)


def test_path_of_three_has_the_shortest_update_list(esp, model):
    st, want = check_all(esp, model, from_scipy(esp, L.path(3)), 1)
    assert st["nodes"] == 3 and st["deepest"] == 1


def test_path(esp, model):
    st, _ = check_all(esp, model, from_scipy(esp, L.path(100)), 8)
    assert st["deepest"] >= 4 and st["largest_node"] <= 8


def test_block_diagonal(esp, model):
    """six 7 x 5 grids and five 3-paths, leaf_size 4: several roots"""
    st, _ = check_all(esp, model, from_scipy(esp, L.block_diagonal()), 4)
    assert st["nodes"] > 11


def test_nonsymmetric_stored_pattern(esp, model):
    """entries stored one way only, the values of the two triangles unrelated: the upper triangle is what is factorized (it is
    diagonally dominant with a positive diagonal), the strict lower triangle only shapes the graph"""
    S = L.random_pattern(300, False, 0.01, 7)
    assert ((S != 0) != (S != 0).T).nnz > 0
    check_all(esp, model, from_scipy(esp, S))
    T = sp.csc_matrix(S, copy=True)
    T.sort_indices()
    col = np.repeat(np.arange(300), np.diff(T.indptr))
    T.data[T.indices > col] = np.nan                                        # garbage below the diagonal: no bit of L changes
    A, B = from_scipy(esp, S), from_scipy(esp, T)
    P, Q = esp.CholeskyFactorization(A), esp.CholeskyFactorization(B)
    assert same_bits(P.factor()[2], Q.factor()[2])
    P.close()
    Q.close()


# ---- tile and block edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 1023, 1024, 1025])
def test_dense_node_widths(esp, model, n):
    A = esp.fdrand(n, 1, 1)
    st, want = check_all(esp, model, A, 16, 0)
    assert (st["nodes"], st["largest_node"], st["panel_doubles"]) == (1, n, n * n)
    assert (st["small_nodes"], st["wide_nodes"]) == ((1, 0) if n <= 32 else (0, 1))
    if n in (33, 65, 161):                                                  # the other form on the same node
        st2, _ = check_all(esp, model, A, 16, 0, wide_from=EVERYTHING_SMALL)
        assert (st2["small_nodes"], st2["wide_nodes"]) == (1, 0)
    if n in (2, 31, 32):
        st2, _ = check_all(esp, model, A, 16, 0, wide_from=1)
        assert (st2["small_nodes"], st2["wide_nodes"]) == (0, 1)


@pytest.mark.parametrize("k", [15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_separator_widths(esp, model, k):
    st, want = check_all(esp, model, esp.fdrand(k, k, 1))
    top = want.nsize[want.level[want.c] == 0]
    assert len(top) == k and np.all(top == k)                                # the top separator: one node, k wide


def struct_lengths(F):
    return [int(F.lcp[s + 1] - F.lcp[s] - F.nsize[s]) for s in np.unique(F.nstart)]


@pytest.mark.parametrize("rows,nx,ny", [(63, 61, 64), (64, 47, 94), (65, 63, 66)])
def test_struct_heights_at_the_row_tile_edge(esp, model, rows, nx, ny):
    A = from_scipy(esp, L.dominant(L.edges_pattern(nx * ny, L.grid_edges(nx, ny))))
    st, want = check_all(esp, model, A, 4)
    assert max(struct_lengths(want)) == rows


# ---- both forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,leaf", [((10, 10, 10), 16), ((33, 33, 1), 32)])
def test_both_forms_give_the_same_bits(esp, model, grid, leaf):
    A = esp.fdrand(*grid)
    lib, h = A._d.lib, A._d.h
    want = model.cholesky(host_arrays(A), leaf)
    got = {}
    for wide_from in (1, EVERYTHING_SMALL):
        assert lib.esp_debug_cholesky_wide_from(h, wide_from) == 0
        P = esp.CholeskyFactorization(A, leaf)
        st = P.stats()
        if wide_from == 1:
            assert st["small_nodes"] == 0 and st["wide_nodes"] == st["nodes"]
        else:
            assert st["wide_nodes"] == 0 and st["small_nodes"] == st["nodes"] and st["wide_block_columns"] == 0
        check_order(P, want)
        check_numeric(P, want)
        got[wide_from] = P.factor()[2]
        P.close()
    assert lib.esp_debug_cholesky_wide_from(h, 0) == 0 and lib.esp_debug_cholesky_wide_from(h, -1) == ESP_ERR_INVALID
    assert same_bits(got[1], got[EVERYTHING_SMALL])


# ---- updates -------------------------------------------------------------------------------------------------------------------------------
def test_values_only_update_equals_fresh_create(esp, model):
    A = esp.fdrand(5, 4, 3)
    P = esp.CholeskyFactorization(A, 8)
    launches = P.stats()["ordering_launches"]
    assert launches > 0
    v = np.random.default_rng(6).standard_normal(A.n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: the panels hold the values of the last update!
    P.update()
    assert P.stats()["ordering_launches"] == launches     # the ordering was not run again
    want = model.cholesky(host_arrays(A), 8)
    F = esp.CholeskyFactorization(A, 8)
    for Q in (P, F):
        check_order(Q, want)
    u_new = check_numeric(P, want, seed=6)
    assert same_bits(F.ldiv(v), u_new) and not same_bits(u_new, u_old)
    assert same_bits(P.factor()[2], F.factor()[2])
    F.close()
    P.close()


def test_pattern_change_needs_update_and_rebuilds(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.CholeskyFactorization(A, 8)
    launches = P.stats()["ordering_launches"]
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.25, 0.25])       # two corners
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.cg(A, v, Pl=P), P.permutation, P.tree, P.factor):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    assert P.stats()["ordering_launches"] > launches       # everything anew
    want = model.cholesky(host_arrays(A), 8)
    check_order(P, want)
    u = check_numeric(P, want, seed=6)
    F = esp.CholeskyFactorization(A, 8)
    assert same_bits(F.ldiv(v), u)
    F.close()
    P.close()


# ---- launch counts ---------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(esp):
    A = esp.fdrand(10, 10, 10)
    P = esp.CholeskyFactorization(A, 16)
    st = P.stats()
    assert st["wide_nodes"] > 0 and st["small_nodes"] > 0
    assert 0 < st["ldiv_launches"] <= 4 * (st["deepest"] + 1) + 2
    assert 0 < st["factor_launches"] <= 1 + (st["deepest"] + 1) + 2 * st["wide_block_columns"]
    print("10x10x10, leaf 16: %s" % st)
    P.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, leaf=32, depth=48):
    p = C.c_void_p()
    rc = lib.esp_precon_cholesky_create(h, leaf, depth, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def indefinite(esp, how):
    cp, rv, nz = host_arrays(esp.fdrand(6, 5, 1))
    col = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
    d = int(np.flatnonzero((rv - 1 == col) & (col == 17))[0])
    if how == "negated":
        nz[d] = -nz[d]
        return cp, rv, nz
    cp[18:] -= 1
    return cp, np.delete(rv, d), np.delete(nz, d)


@pytest.mark.parametrize("how", ["negated", "removed"])
@pytest.mark.parametrize("wide_from", [0, 1])
def test_not_positive_definite_on_create(esp, model, how, wide_from):
    csc = indefinite(esp, how)
    with pytest.raises(CM.NotPosDef) as want:
        model.cholesky(csc, 4)
    A = from_arrays(esp, *csc)
    assert A._d.lib.esp_debug_cholesky_wide_from(A._d.h, wide_from) == 0
    with pytest.raises(esp.PosDefError) as e:
        esp.CholeskyFactorization(A, 4)
    assert isinstance(e.value, esp.EspError) and e.value.code == ESP_ERR_NOTPOSDEF
    assert "position %d in c" % (want.value.position + 1) in str(e.value) and "A's column is %d)" % (want.value.column + 1) in str(e.value)
    assert A._d.lib.esp_destroy(A._d.h) == 0                                # the failed create left nothing bound to h
    A._d.h = None


def test_not_positive_definite_on_update_then_repaired(esp, model):
    A = esp.fdrand(6, 5, 1)
    P = esp.CholeskyFactorization(A, 4)
    v = np.random.default_rng(3).standard_normal(A.n)
    good = A.sparse().nzval.copy()
    csc = A.sparse()
    col = np.repeat(np.arange(A.n), np.diff(csc.colptr))
    d = int(np.flatnonzero((np.asarray(csc.rowval) - 1 == col) & (col == 17))[0])
    csc.nzval[d] = -csc.nzval[d]
    A._push_edits()
    with pytest.raises(CM.NotPosDef) as want:
        model.cholesky(host_arrays(A), 4)
    with pytest.raises(esp.PosDefError) as e:
        P.update()
    assert "A's column is %d)" % (want.value.column + 1) in str(e.value)
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    A.sparse().nzval[:] = good                                              # (handed out again: the edit goes up with the update)
    P.update()
    check_numeric(P, model.cholesky(host_arrays(A), 4))
    P.close()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for leaf, depth in ((0, 48), (-3, 48), (32, -1), (32, 65)):
        assert raw_create(lib, h, leaf, depth)[0] == ESP_ERR_INVALID
    p = C.c_void_p()
    assert lib.esp_precon_cholesky_create(None, 32, 48, C.byref(p)) == ESP_ERR_INVALID
    assert lib.esp_precon_cholesky_create(h, 32, 48, None) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h)[0] == ESP_ERR_INVALID
    one, val = np.ones(1, np.int64), np.ones(1)                                              # pending entries
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # no inner kind of Block or Colored
    ptr, idx = np.array([1, 5], np.int64), np.arange(1, 5, dtype=np.int64)
    assert lib.esp_precon_block_create(h, esp.ESP_PRECON_CHOLESKY, 1, ptr.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 0,
                                       C.byref(p)) == ESP_ERR_INVALID
    assert lib.esp_precon_colored_create(h, esp.ESP_PRECON_CHOLESKY, C.byref(p)) == ESP_ERR_INVALID
    # the accessors of the other kinds refuse it and the other way round; get_factor / levels / launches answer as for AMG
    rc, p, _ = raw_create(lib, h)
    assert rc == 0
    b = C.c_void_p()
    out = (C.c_int64 * 12)()
    assert lib.esp_precon_lu_matrix(p, C.byref(b)) == ESP_ERR_INVALID and lib.esp_precon_lu_stats(p, out) == ESP_ERR_INVALID
    buf = np.zeros(64)
    assert lib.esp_precon_get_factor(p, buf.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_INVALID
    assert lib.esp_precon_levels(p, out) == 0 and list(out[:3]) == [0, 0, 0]
    assert lib.esp_precon_launches(p, out) == 0 and list(out[:6]) == [0] * 6
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 2, C.byref(q)) == 0
    assert lib.esp_precon_cholesky_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_cholesky_perm(q, out, 0) == ESP_ERR_INVALID
    assert lib.esp_precon_cholesky_tree(q, None, None, 0) == ESP_ERR_INVALID
    assert lib.esp_precon_cholesky_factor(q, None, None, None, 0) == ESP_ERR_INVALID
    assert lib.esp_precon_destroy(q) == 0
    assert lib.esp_destroy(h) == ESP_ERR_STATE                                               # a live factorization
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.CholeskyFactorization(A)
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
    """the device's free memory, read through the runtime, must not keep falling over 50 create / update / destroy cycles"""
    import torch
    A = esp.fdrand(8, 7, 6)

    def cycle(k):
        for _ in range(k):
            P = esp.CholeskyFactorization(A, 8)
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(50)
    assert free0 - free1 < (8 << 20), (free0, free1)


# ---- the reference's acceptance tests (test/test_default_cholesky.jl: test_lu1 / test_lu2 with CholeskyFactorization) ---------------------
def add_to_diagonal(esp, A, by):
    d = np.arange(1, A.n + 1)
    A.append(esp.ESP_UPDATE, d, d, np.full(A.n, by))
    A.flush()


GRIDS = [(10, 10, 10), (25, 40, 1), (1000, 1, 1)]


@pytest.mark.parametrize("grid", GRIDS)
def test_reference_lu1(esp, grid):
    A = esp.fdrand(*grid, rand_mode=0)
    b = np.random.default_rng(11).random(A.n)
    F = esp.cholesky(A)
    assert isinstance(F, esp.CholeskyFactorization) and esp.issolver(F) and esp.issolver(esp.CholeskyFactorization)
    assert esp.lu_(F, A) is F
    x1 = F.solve(b)
    arrays = host_arrays(A)
    a1 = sp.csc_matrix((arrays[2], arrays[1] - 1, arrays[0] - 1), shape=(A.n, A.n)).toarray()
    add_to_diagonal(esp, A, 1.0)
    launches = F.stats()["ordering_launches"]
    assert esp.factorize_(F, A) is F and F.stats()["ordering_launches"] == launches
    x2 = F.solve(b)
    a2 = a1 + np.eye(A.n)
    for x, a in ((x1, a1), (x2, a2)):
        ref = np.linalg.solve(a, b)
        assert np.linalg.norm(ref - x) / np.linalg.norm(ref) <= 100.0 * np.sqrt(EPS)
    F.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_reference_lu2(esp, grid):
    A = esp.fdrand(*grid, rand_mode=0)
    n = A.n
    b = np.random.default_rng(12).random(n)
    F = esp.cholesky(A)
    x1 = F.solve(b)
    i = np.arange(4, n - 3 + 1)
    A.append(esp.ESP_UPDATE, np.concatenate([i, i - 3]), np.concatenate([i + 3, i]), np.full(2 * len(i), -1.0e-4))
    A.flush()
    nnz_l = F.stats()["nnz"]
    assert esp.lu_(F, A) is F and F.stats()["nnz"] > nnz_l
    x2 = F.solve(b)
    assert np.all(x1 < x2)
    B = esp.fdrand(*grid, rand_mode=0)
    assert esp.cholesky_(F, B) is F and F.A is B and same_bits(F.solve(b), x1)
    F.close()


# ---- solvers ---------------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! driven with the Cholesky model's ldiv and A's mul"""

    def __init__(self, lib, fact):
        self.m, self.P, self.csc, self.n = lib, fact, fact.csc, fact.n

    def ldiv(self, v):
        return self.P.ldiv(np.ascontiguousarray(v, np.float64))


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


@pytest.mark.parametrize("where", ["host", "torch"])
def test_solvers(esp, model, solver_lib, gmres_lib, where):
    A = esp.fdrand(6, 5, 4)
    n = A.n
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.CholeskyFactorization(A, 8)
    M = SolverModel(solver_lib, model.cholesky(arrays, 8))
    x, log = esp.cg(A, dev(b), Pl=P, log=True)
    wx, wh, wit, wconv = M.cg(b)
    assert log["iters"] == wit and log["isconverged"] == wconv and wconv and wit <= 2
    assert same_bits(history_of(log), wh) and same_bits(host(x), wx)
    x, log = esp.gmres(A, dev(b), Pl=P, restart=20, log=True)
    want = gmres_lib.gmres_cb(M, n, b, restart=20)
    assert (log["iters"], log["mvps"], log["reorth"], log["isconverged"]) == (want.iters, want.mvps, want.reorth, want.converged)
    assert want.converged and same_bits(history_of(log), want.history) and same_bits(host(x), want.x)
    u0 = np.random.default_rng(12).standard_normal(n)
    got, log = esp.simple(A, dev(b), u=dev(u0.copy()), Pl=P, maxiter=3, reltol=0.0, log=True)
    wu, wh, wit = M.simple(b, u=u0, maxiter=3, reltol=0.0)
    assert wit == 3 and same_bits(host(got), wu) and same_bits(log["resnorm"], wh)
    # (an exact Pl leaves BiCGStab(l) nothing to minimise after its first step, as tests/test_lu_gpu.py records for LU: the model's
    # own outcome is asserted, whatever it is)
    x, log = esp.bicgstabl(A, dev(b), l=2, Pl=P, log=True)
    wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2)
    assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv)
    assert same_bits(history_of(log), wh) and same_bits(host(x), wx)
    P.close()


def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    for kw in ({"leaf_size": 0}, {"leaf_size": 1.5}, {"max_depth": -1}, {"max_depth": 65}):
        with pytest.raises(ValueError):
            esp.CholeskyFactorization(A, **kw)
    P = esp.cholesky(A, leaf_size=8)
    assert (P.leaf_size, P.max_depth) == (8, 48) and set(P.stats()) >= {"nnz", "factor_launches", "ldiv_launches", "small_nodes", "wide_nodes"}
    b = A.mul(np.ones(A.n))
    assert np.linalg.norm(P.solve(b) - 1.0) <= 1e-12 * np.sqrt(A.n)
    assert not isinstance(A.solve(b), type(None)) and isinstance(esp.lu(A), esp.LUFactorization)       # A \ b stays LU
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.CholeskyFactorization)
    with pytest.raises(TypeError):
        esp.ColoredPreconditioner(A, esp.CholeskyFactorization)
    with pytest.raises(TypeError):
        esp.cholesky_(esp.lu(A), A)
    P.close()
    with pytest.raises(ValueError):
        P.solve(b)
