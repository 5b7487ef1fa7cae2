"""GPU: LUFactorization(form="panels") (include/esparse_hip.h, esp_precon_lu_create_form) against tests/lu_model.c and
iluam_model.c over B (lu_modellib: B, fval, ldiv), bit for bit, a NaN equal to a NaN at the same position: the permutation, the tree,
fill_matrix(), factor(), ldiv! on host vectors, device vectors and in place, solve; both forms of the numeric factorization
(wide_from = 0, the default, and = 1, everything wide; the dense nodes also with everything small), the column form on the device
itself, update!, the launch counts, the error codes, the solvers, the reference's acceptance tests.

The tile and block dimensions T of csrc/lu_panels.hip (csrc/panels.hpp) and the sizes that straddle them:
  NB = 32      columns of the update tile = the factor block width = W_small (the wide form starts at width 33)
  KB = 16      columns of a descendant (or of the node itself) staged in LDS at once
  TR = 64      rows of the update tile, of PL and of PU alike
  FR = 128     rows below the diagonal block one workgroup finishes (rows below the first block column: width - 32)
  CT = 256     lanes of a workgroup: the rows one pass of the solves takes
  TRI_LDS = 1024  rows of a node's triangle the solves keep in LDS (a wider node uses a second vector)
Node widths T - 1, T, T + 1 are dense nodes: fdrand n x 1 x 1 with max_depth = 0 (one leaf of width n, h = 0), n in
  1, 2 | 15, 16, 17 | 31, 32, 33 | 63, 64, 65 | 127, 128, 129 | 159, 160, 161 (128 rows below the first block) | 255, 256, 257
  | 1023, 1024, 1025.
Separator widths at the same edges: k x k x 1 grids, k in 15, 16, 17, 31, 32, 33, 63, 64, 65.
Struct heights at the row-tile edge: the 2-D grids 61 x 64, 47 x 94, 63 x 66 with leaf_size 4, whose longest struct list holds
  63 / 64 / 65 rows (asserted on the model's lists).
Update lists: length 0 (every leaf), 2 (a path of 3 with leaf_size 1) and 199 (the arrow's hub).  Structural zeros that differ
  between PL and PU: the non-symmetric stored pattern and star(entries), entries in 32, 33, 65.

The launch bound of the numeric factorization (test_launch_counts): one load launch; per depth one launch for all its small nodes
(if any) and two launches (tiles + diagonal blocks, rows below and right) per block column of its widest wide node:
  factor_launches <= 1 + (deepest + 1) + 2 * wide_block_columns,
wide_block_columns = the sum over the depths of ceil(width of the widest wide node / 32), which panel_stats() reports.  One ldiv!:
a gather, one forward and one backward launch per depth, a scatter: ldiv_launches <= 4 * (deepest + 1) + 2."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
import lu_modellib as L
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6
ESP_LU_COLUMNS, ESP_LU_PANELS = 0, 1
EPS = np.finfo(np.float64).eps
EVERYTHING_SMALL = 2 ** 30


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return L.Model(tmp_path_factory.mktemp("lu_panels_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("lu_panels_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("lu_panels_gmres_model"))


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


def convdiff(esp, nx, ny, nz, pe):
    I, J, V = convdiff_triplets(nx, ny, nz, pe)
    A = esp.ExtendableSparseMatrix(nx * ny * nz, nx * ny * nz)
    A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def signs(f):
    """(the sign bits set among the entries that are no NaN, the NaNs): a NaN's own sign is the hardware's choice -- the host's
    0/0 is negative, the device's positive -- and same_bits leaves it out for the same reason"""
    f = np.asarray(f, np.float64)
    return int(np.signbit(f[~np.isnan(f)]).sum()), int(np.isnan(f).sum())


def wide_from(A, w):
    assert A._d.lib.esp_debug_lu_wide_from(A._d.h, w) == 0


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


def check_bounds(P):
    st, ps = P.stats(), P.panel_stats()
    assert ps["small_nodes"] + ps["wide_nodes"] == st["nodes"]
    if P.A.n:
        assert 0 < ps["ldiv_launches"] <= 4 * (st["deepest"] + 1) + 2
        assert 0 < ps["factor_launches"] <= 1 + (st["deepest"] + 1) + 2 * ps["wide_block_columns"]
    return ps


def check_numeric(P, want, seed=1, u=None):
    n = want.n
    assert same_bits(P.factor(), want.fval)
    assert P.levels() == (0, 0, 0) and P.launches() == ((0, 0),) * 3
    v = np.random.default_rng(seed).standard_normal(n)
    if u is None:
        u = want.ldiv(v)
    assert same_bits(P.ldiv(v), u) and same_bits(P.solve(v), u)
    t = to_device(v)
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    assert same_bits(P.ldiv(to_device(v)).cpu().numpy(), u)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, u)
    return u


def check_all(esp, model, A, leaf_size=32, max_depth=48, wides=(0, 1), want=None):
    """every wide_from of `wides` against ONE model run -> ({wide_from: panel_stats}, want)"""
    want = want if want is not None else model.lu(host_arrays(A), leaf_size, max_depth)
    out, u = {}, None
    try:
        for w in wides:
            wide_from(A, w)
            P = esp.LUFactorization(A, leaf_size, max_depth, form="panels")
            try:
                check_order(P, want)
                u = check_numeric(P, want, u=u)
                out[w] = check_bounds(P)
                out[w]["nodes"] = P.stats()["nodes"]
            finally:
                P.close()
    finally:
        wide_from(A, 0)
    if 1 in out:
        assert out[1]["small_nodes"] == 0 and out[1]["wide_nodes"] == out[1]["nodes"]
    if EVERYTHING_SMALL in out:
        assert out[EVERYTHING_SMALL]["wide_nodes"] == 0 and out[EVERYTHING_SMALL]["wide_block_columns"] == 0
    return out, want


# ---- matrix shapes ---------------------------------------------------------------------------------------------------------------------
def test_empty_one_and_diagonal(esp, model):
    E = esp.ExtendableSparseMatrix(0, 0)
    P = esp.LUFactorization(E, form="panels")
    ps = P.panel_stats()
    assert P.stats()["nnz"] == 0 and ps["ldiv_launches"] == 0 and ps["factor_launches"] == 0 and ps["panel_doubles"] == 0
    assert len(P.permutation()) == 0 and len(P.ldiv(np.empty(0))) == 0 and len(P.factor()) == 0
    P.update()
    P.close()
    st, _ = check_all(esp, model, from_scipy(esp, sp.csc_matrix(np.array([[4.0]]))))
    assert st[0]["panel_doubles"] == 2
    st, want = check_all(esp, model, from_scipy(esp, sp.diags(np.arange(1.0, 501.0))))       # 500 nodes of width 1, h = 0
    assert (want.stats["nodes"], st[0]["panel_doubles"], st[0]["small_nodes"]) == (500, 1000, 500)


def test_path_of_three_has_the_shortest_update_list(esp, model):
    st, want = check_all(esp, model, from_scipy(esp, L.path(3)), 1)
    assert want.stats["nodes"] == 3 and want.stats["deepest"] == 1


def test_arrow(esp, model):
    """width-1 leaves with h = 1, and the hub's update list of 199 descendants"""
    st, want = check_all(esp, model, from_scipy(esp, L.arrow(200)))
    assert want.stats["nnz"] == 200 + 2 * 199 and want.stats["rounds"] == 2


def test_block_diagonal(esp, model):
    """six 7 x 5 grids and five 3-paths, leaf_size 4: several roots"""
    st, want = check_all(esp, model, from_scipy(esp, L.block_diagonal()), 4)
    assert want.stats["nodes"] > 11


def test_nonsymmetric_stored_pattern(esp, model):
    """entries stored one way only: B holds +0.0 where only the mirror is stored, PL and PU get different structural zeros"""
    S = L.random_pattern(300, False, 0.01, 7)
    assert ((S != 0) != (S != 0).T).nnz > 0
    check_all(esp, model, from_scipy(esp, S))
    check_all(esp, model, from_scipy(esp, S), 4)


@pytest.mark.parametrize("entries", [32, 33, 65])
def test_star(esp, model, entries):
    """the hub's column holds `entries` stored rows, its row the diagonal alone: PU of every spoke is all fill"""
    check_all(esp, model, from_scipy(esp, L.star(entries)))
    check_all(esp, model, from_scipy(esp, L.star(entries)), 16, 0, wides=(0, 1, EVERYTHING_SMALL))


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 1023, 1024, 1025])
def test_dense_node_widths(esp, model, n):
    st, want = check_all(esp, model, esp.fdrand(n, 1, 1), 16, 0, wides=(0, 1, EVERYTHING_SMALL))
    assert (want.stats["nodes"], want.stats["largest_node"], st[0]["panel_doubles"]) == (1, n, 2 * n * n)
    assert (st[0]["small_nodes"], st[0]["wide_nodes"]) == ((1, 0) if n <= 32 else (0, 1))
    assert st[1]["wide_block_columns"] == (n + 31) // 32


@pytest.mark.parametrize("k", [15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_separator_widths(esp, model, k):
    st, want = check_all(esp, model, esp.fdrand(k, k, 1))
    top = want.nsize[want.level[want.c] == 0]
    assert len(top) == k and np.all(top == k)                                # the top separator: one node, k wide


def struct_lengths(F):
    bcp, brv, _ = F.B
    return [int(np.count_nonzero(brv[bcp[s] - 1:bcp[s + 1] - 1] - 1 >= s + F.nsize[s])) for s in np.unique(F.nstart)]


@pytest.mark.parametrize("rows,nx,ny", [(63, 61, 64), (64, 47, 94), (65, 63, 66)])
def test_struct_heights_at_the_row_tile_edge(esp, model, rows, nx, ny):
    A = from_scipy(esp, L.dominant(L.edges_pattern(nx * ny, L.grid_edges(nx, ny))))
    st, want = check_all(esp, model, A, 4)
    assert max(struct_lengths(want)) == rows


# ---- workloads, and the column form on the device ----------------------------------------------------------------------------------------
def test_workload_20x20(esp, model):
    check_all(esp, model, esp.fdrand(20, 20, 1), wides=(0, 1, EVERYTHING_SMALL))


@pytest.mark.parametrize("which", ["fd10x10x10", "convdiff"])
def test_workloads_and_both_device_forms(esp, model, which):
    """fdrand 10 x 10 x 10 with leaf_size 16 and the convection-diffusion matrix (non-symmetric values): the model, and the column
    form on the device itself -- equal factor() and ldiv bits"""
    A, leaf = (esp.fdrand(10, 10, 10), 16) if which == "fd10x10x10" else (convdiff(esp, 6, 5, 4, 2.0), 8)
    st, want = check_all(esp, model, A, leaf, wides=(0, 1, EVERYTHING_SMALL))
    if which == "fd10x10x10":
        assert st[0]["wide_nodes"] > 0 and st[0]["small_nodes"] > 0
        print("10x10x10, leaf 16: %s" % st[0])
    Pc, Pp = esp.LUFactorization(A, leaf), esp.LUFactorization(A, leaf, form="panels")
    assert (Pc.form, Pp.form) == ("columns", "panels")
    assert same_bits(Pp.factor(), Pc.factor()) and np.array_equal(Pp.permutation(), Pc.permutation())
    v = to_device(np.random.default_rng(3).standard_normal(A.n))
    assert same_bits(Pp.ldiv(v).cpu().numpy(), Pc.ldiv(v).cpu().numpy())
    assert Pc.levels() != (0, 0, 0) and Pc.stats() == Pp.stats()
    Pc.close()
    Pp.close()


def test_stored_zeros_and_nan(esp, model):
    """stored 0.0, -0.0 and NaN off-diagonals in a 5 x 4 x 3 grid: the model, in both forms; the sign bits of factor() are the
    model's (a predicate replaced by a multiply with zero turns -0.0 into +0.0)"""
    cp, rv, nz = host_arrays(esp.fdrand(5, 4, 3))
    off = [q for j in range(len(cp) - 1) for q in range(cp[j] - 1, cp[j + 1] - 1) if rv[q] != j + 1]
    nz[off[3]], nz[off[10]], nz[off[17]] = 0.0, -0.0, np.nan
    A = from_arrays(esp, cp, rv, nz)
    for leaf in (4, 32):
        want = model.lu((cp, rv, nz), leaf)
        assert np.isnan(want.fval).any()
        for w in (0, 1, EVERYTHING_SMALL):
            wide_from(A, w)
            P = esp.LUFactorization(A, leaf, form="panels")
            check_order(P, want)
            check_numeric(P, want)
            assert signs(P.factor()) == signs(want.fval)
            P.close()
    wide_from(A, 0)


def test_zero_pivot_gives_the_models_inf_and_nan(esp, model):
    """no pivot test: a leaf whose second pivot cancels to 0.0 exactly propagates Inf and NaN as the column form does"""
    S = L.path(12).tolil()
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = 2.0, 4.0, 1.0, 2.0
    A = from_scipy(esp, S.tocsc())
    st, want = check_all(esp, model, A, 4, wides=(0, 1, EVERYTHING_SMALL))
    assert not np.isfinite(want.fval).all()
    Pc, Pp = esp.LUFactorization(A, 4), esp.LUFactorization(A, 4, form="panels")
    assert same_bits(Pp.factor(), Pc.factor()) and signs(Pp.factor()) == signs(Pc.factor()) == signs(want.fval)
    Pc.close()
    Pp.close()


# ---- updates -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 1])
def test_values_only_update_equals_fresh_create(esp, model, w):
    A = esp.fdrand(5, 4, 3)
    wide_from(A, w)
    P = esp.LUFactorization(A, 8, form="panels")
    launches = P.stats()["launches"]
    assert launches > 0
    v = np.random.default_rng(6).standard_normal(A.n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: the values of the last update!
    P.update()
    assert P.stats()["launches"] == launches              # the ordering was not run again
    want = model.lu(host_arrays(A), 8)
    F = esp.LUFactorization(A, 8, form="panels")
    for Q in (P, F):
        check_order(Q, want)
    u_new = check_numeric(P, want, seed=6)
    assert same_bits(F.ldiv(v), u_new) and not same_bits(u_new, u_old)
    assert same_bits(P.factor(), F.factor()) and P.panel_stats() == F.panel_stats()
    F.close()
    P.close()
    wide_from(A, 0)


def test_pattern_change_needs_update_and_rebuilds(esp, model):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.LUFactorization(A, 8, form="panels")
    launches = P.stats()["launches"]
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.5, 0.25])       # two corners
    A.flush()
    for call in (lambda: P.ldiv(v), lambda: esp.gmres(A, v, Pl=P), P.permutation, P.tree, P.factor):
        with pytest.raises(esp.EspError) as e:
            call()
        assert e.value.code == ESP_ERR_STATE
    P.update()
    assert P.stats()["launches"] > launches                # everything anew
    want = model.lu(host_arrays(A), 8)
    check_order(P, want)
    u = check_numeric(P, want, seed=6)
    check_bounds(P)
    F = esp.LUFactorization(A, 8, form="panels")
    assert same_bits(F.ldiv(v), u)
    F.close()
    P.close()


def test_launch_counts(esp):
    A = esp.fdrand(10, 10, 10)
    P = esp.LUFactorization(A, 16, form="panels")
    st, ps = P.stats(), check_bounds(P)
    assert ps["wide_nodes"] > 0 and ps["small_nodes"] > 0
    assert ps["ldiv_launches"] == 2 * (st["deepest"] + 1) + 2
    assert P.levels() == (0, 0, 0) and P.launches() == ((0, 0),) * 3
    P.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, leaf=32, depth=48, form=ESP_LU_PANELS):
    p = C.c_void_p()
    rc = lib.esp_precon_lu_create_form(h, leaf, depth, form, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for form in (-1, 2, 7):
        rc, p, _ = raw_create(lib, h, form=form)
        assert rc == ESP_ERR_INVALID and not p.value
    for leaf, depth in ((0, 48), (-3, 48), (32, -1), (32, 65)):
        assert raw_create(lib, h, leaf, depth)[0] == ESP_ERR_INVALID
    p = C.c_void_p()
    assert lib.esp_precon_lu_create_form(None, 32, 48, 1, C.byref(p)) == ESP_ERR_INVALID
    assert lib.esp_precon_lu_create_form(h, 32, 48, 1, None) == ESP_ERR_INVALID
    assert lib.esp_debug_lu_wide_from(None, 1) == ESP_ERR_INVALID and lib.esp_debug_lu_wide_from(h, -1) == ESP_ERR_INVALID
    R = esp.ExtendableSparseMatrix(4, 5)                                                       # rectangular
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h)[0] == ESP_ERR_INVALID
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))   # no stored (3,3)
    rc, _, msg = raw_create(M._d.lib, M._d.h)
    rc0, _, msg0 = raw_create(M._d.lib, M._d.h, form=ESP_LU_COLUMNS)
    assert rc == rc0 == ESP_ERR_INVALID and msg == msg0 and "diagonal" in msg and "A's column is 3" in msg
    # form 0 through the new entry point is the column form; panel_stats refuses it, and every other kind
    out = (C.c_int64 * 6)()
    rc, pc, _ = raw_create(lib, h, form=ESP_LU_COLUMNS)
    assert rc == 0 and lib.esp_precon_lu_panel_stats(pc, out) == ESP_ERR_INVALID
    lev = (C.c_int64 * 3)()
    assert lib.esp_precon_levels(pc, lev) == 0 and list(lev) != [0, 0, 0]
    assert lib.esp_precon_destroy(pc) == 0
    q = C.c_void_p()
    assert lib.esp_precon_create(h, 2, C.byref(q)) == 0
    assert lib.esp_precon_lu_panel_stats(q, out) == ESP_ERR_INVALID and lib.esp_precon_destroy(q) == 0
    rc, p, _ = raw_create(lib, h)
    assert rc == 0 and lib.esp_precon_lu_panel_stats(p, out) == 0 and lib.esp_precon_lu_panel_stats(p, None) == ESP_ERR_INVALID
    assert lib.esp_precon_lu_panel_stats(None, out) == ESP_ERR_INVALID
    assert lib.esp_precon_get_factor(p, None, 0) == ESP_ERR_INVALID
    form = C.c_int32(7)
    assert lib.esp_debug_iluam_form(p, 1) == ESP_ERR_INVALID and lib.esp_debug_last_iluam_form(p, C.byref(form)) == ESP_ERR_INVALID
    b = C.c_void_p()
    assert lib.esp_precon_lu_matrix(p, C.byref(b)) == 0 and b.value
    assert lib.esp_destroy(h) == ESP_ERR_STATE                    # the handle refuses destroy while the factorization lives
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_fill_guard_refuses_before_the_panels_are_allocated(esp, model):
    """esp_debug_lu_fill_cap: ESP_ERR_UNSUPPORTED with nnz(B) in the message (the refusal lies in front of the tables and the panels:
    csrc/lu.hip, build_b); a refused update! after a pattern change leaves the earlier factorization and its panels usable"""
    A = esp.fdrand(5, 4, 3)
    lib, h = A._d.lib, A._d.h
    want = model.lu(host_arrays(A))
    assert lib.esp_debug_lu_fill_cap(h, want.stats["nnz"]) == 0
    rc, _, msg = raw_create(lib, h)
    assert rc == ESP_ERR_UNSUPPORTED and str(want.stats["nnz"]) in msg
    assert lib.esp_debug_lu_fill_cap(h, 0) == 0
    P = esp.LUFactorization(A, form="panels")
    launches, ps = P.stats()["launches"], P.panel_stats()
    A.append(esp.ESP_UPDATE, [A.n, 1], [1, A.n], [0.5, 0.25])
    A.flush()
    want2 = model.lu(host_arrays(A))
    assert lib.esp_debug_lu_fill_cap(h, want2.stats["nnz"]) == 0
    with pytest.raises(esp.EspError) as e:
        P.update()                                           # refused before B and the panels are replaced
    assert e.value.code == ESP_ERR_UNSUPPORTED and str(want2.stats["nnz"]) in str(e.value)
    st = P.stats()
    assert st["nnz"] == want.stats["nnz"] and st["launches"] == launches and P.panel_stats() == ps      # the earlier state
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
    P = esp.LUFactorization(A, form="panels")
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
    A = esp.fdrand(8, 7, 6)

    def cycle(k):
        for _ in range(k):
            P = esp.LUFactorization(A, 8, form="panels")
            P.update()
            P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(20)
    assert free0 - free1 < (8 << 20), (free0, free1)


# ---- solvers -------------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! driven with the LU model's ldiv and A's mul"""

    def __init__(self, lib, fact):
        self.m, self.P, self.csc, self.n = lib, fact, fact.csc, fact.n

    def ldiv(self, v):
        return self.P.ldiv(np.ascontiguousarray(v, np.float64))


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg(esp, model, solver_lib, where):
    A = esp.fdrand(5, 4, 3)
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(A.n))
    P = esp.LUFactorization(A, 8, form="panels")
    M = SolverModel(solver_lib, model.lu(arrays, 8))
    x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True)
    wx, wh, wit, wconv = M.cg(b)
    assert log["iters"] == wit and log["isconverged"] == wconv and wconv
    assert same_bits(history_of(log), wh) and same_bits(x if where == "host" else x.cpu().numpy(), wx)
    P.close()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_nonsymmetric_solvers(esp, model, solver_lib, gmres_lib, where):
    """bicgstabl(l = 2), gmres(restart = 20) and simple! (its fused u .-= upd) on the convection-diffusion matrix: the iteration
    counts, histories and solutions of the solver models over the model's ldiv"""
    A = convdiff(esp, 6, 5, 4, 2.0)
    n = A.n
    arrays = host_arrays(A)
    b = solver_lib.mul(arrays, np.ones(n))
    dev = (lambda x: x) if where == "host" else to_device
    host = (lambda x: x) if where == "host" else (lambda x: x.cpu().numpy())
    P = esp.LUFactorization(A, 8, form="panels")
    M = SolverModel(solver_lib, model.lu(arrays, 8))
    x, log = esp.bicgstabl(A, dev(b), l=2, Pl=P, log=True)
    wx, wh, wit, wmv, wconv = M.bicgstabl(b, l=2)
    assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv)
    assert same_bits(history_of(log), wh) and same_bits(host(x), wx)
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
@pytest.mark.parametrize("grid", [(100, 1, 1), (20, 20, 1), (10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_backslash(esp, grid):
    """test/test_backslash.jl through A.solve(b, form="panels") and solve(A, b, form="panels"), host and device vectors"""
    A = esp.fdrand(*grid, rand_mode=0)
    x = np.ones(A.n)
    b = A.mul(x)
    got = A.solve(b, form="panels")
    assert np.linalg.norm(got - x) <= 10.0 * np.sqrt(EPS)
    assert same_bits(esp.solve(A, b, form="panels"), got) and same_bits(A.solve(to_device(b), form="panels").cpu().numpy(), got)
    if A.n < 1000:
        assert same_bits(A.solve(b), got)                                   # the default form: the same bits


def add_to_diagonal(esp, A, by):
    d = np.arange(1, A.n + 1)
    A.append(esp.ESP_UPDATE, d, d, np.full(A.n, by))
    A.flush()


@pytest.mark.parametrize("grid", [(100, 1, 1), (20, 20, 1), (10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu1(esp, grid):
    """test/test_lu.jl:7-31 through lu / lu_ / factorize_: both answers agree with a dense solve to 100 sqrt(eps), relative"""
    A = esp.fdrand(*grid, rand_mode=0)
    b = np.random.default_rng(11).random(A.n)
    F = esp.lu(A, form="panels")
    assert esp.issolver(F) and esp.lu_(F, A) is F and F.form == "panels"
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
    assert same_bits(A.solve(b, form="panels"), x2)
    F.close()


@pytest.mark.parametrize("grid", [(100, 1, 1), (20, 20, 1), (10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu2(esp, grid):
    """test/test_lu.jl:33-45: after A[i,i+3] -= 1e-4, A[i-3,i] -= 1e-4 (a pattern change) and lu_, every component of the new
    solution exceeds the old one; lu_ with another matrix binds the factorization anew, in the object's form"""
    A = esp.fdrand(*grid, rand_mode=0)
    n = A.n
    b = np.random.default_rng(12).random(n)
    F = esp.lu(A, form="panels")
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
    assert F.form == "panels" and isinstance(F.panel_stats(), dict)
    F.close()


# ---- Python ----------------------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(5, 4, 3)
    for form in ("panel", "", None, 1):
        with pytest.raises(ValueError):
            esp.LUFactorization(A, form=form)
        with pytest.raises(ValueError):
            A.solve(np.ones(A.n), form=form)
    P = esp.SparspakLU(A, form="panels")
    assert isinstance(P, esp.LUFactorization) and esp.issolver(P) and (P.leaf_size, P.max_depth, P.form) == (32, 48, "panels")
    assert set(P.panel_stats()) == {"panel_doubles", "factor_launches", "ldiv_launches", "small_nodes", "wide_nodes", "wide_block_columns"}
    for call in (lambda: P.debug_factor_form(1), P.last_factor_form):
        with pytest.raises(esp.EspError):
            call()
    b = A.mul(np.ones(A.n))
    assert np.linalg.norm(P.solve(b) - 1.0) <= 1e-12 * np.sqrt(A.n)
    for solve in (esp.cg, esp.gmres, esp.bicgstabl, esp.simple):
        assert np.linalg.norm(solve(A, b, Pl=P) - 1.0) <= 1e-6 * np.sqrt(A.n)
    Q = esp.LUFactorization(A)
    assert Q.form == "columns" and Q.last_factor_form() in (1, 2)
    with pytest.raises(esp.EspError):
        Q.panel_stats()
    Q.close()
    P.close()
    with pytest.raises(ValueError):
        P.panel_stats()
