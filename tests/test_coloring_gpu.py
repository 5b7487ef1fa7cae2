"""GPU: the multicolour ordering on the device (include/esparse_hip.h: esp_graph_coloring, esp_precon_colored_create) against the
normative model of tests/coloring_model.c: colours, permutation and A[c,c] exactly, ldiv! / the ILUAM factor / the level counts
and x, history and counters of simple!, cg, bicgstabl and gmres bit for bit the model preconditioner's (block_precon_modellib's
BlockModel over the single partition c: precon_model.c / iluam_model.c on A[c,c] with v[c], scattered back)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
from bicgstabl_modellib import convdiff_triplets
from coloring_modellib import AMG_LONG, Model, colored_model, dominant_nonsymmetric, replay_pair
from iluam_modellib import level_schedules
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6
KINDS = ["ilu0", "iluam"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("coloring_model"))


@pytest.fixture(scope="module")
def bmodel(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("coloring_block_model"))


@pytest.fixture(scope="module")
def gmodel(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("coloring_gmres_model"))


def factorization(esp, kind):
    return {"ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}[kind]


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
    """a matrix with exactly S's stored entries, through the CSC constructor"""
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


def bidiagonal(esp, n, lower):
    off = -1.0 - 0.001 * np.arange(n - 1)
    return from_scipy(esp, sp.diags([off, 4.0 + 0.001 * np.arange(n)], [-1 if lower else 1, 0]))


def random_nonsymmetric(esp, n, seed=5):
    """a seeded random non-symmetric pattern with a full diagonal, about five entries per column, strictly diagonally dominant"""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=4.0 / n, random_state=rng, data_rvs=rng.standard_normal, format="lil")
    S.setdiag(0.0)
    S = sp.csc_matrix(S)
    S.eliminate_zeros()
    d = 1.0 + np.maximum(np.asarray(abs(S).sum(0)).ravel(), np.asarray(abs(S).sum(1)).ravel())
    return from_scipy(esp, S + sp.diags([d], [0]))


def arrow(esp, n):
    """the first row and the first column full, plus the diagonal"""
    rng = np.random.default_rng(9)
    r = np.arange(1, n)
    I = np.concatenate([np.arange(n), r, np.zeros(n - 1, np.int64)])
    J = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64), r])
    V = np.concatenate([10.0 + rng.random(n), 0.001 * rng.standard_normal(2 * (n - 1))])
    return from_scipy(esp, sp.csc_matrix((V, (I, J)), shape=(n, n)))


def dense(esp, n):
    rng = np.random.default_rng(10)
    M = 0.01 * rng.standard_normal((n, n))
    np.fill_diagonal(M, 2.0 + rng.random(n))
    return from_scipy(esp, sp.csc_matrix(M))


SHAPES = {
    "n1": lambda esp: from_scipy(esp, sp.csc_matrix(np.array([[4.0]]))),
    "n2": lambda esp: from_scipy(esp, sp.csc_matrix(np.array([[4.0, -1.0], [-2.0, 5.0]]))),
    "diagonal5": lambda esp: from_scipy(esp, sp.diags([2.0 + np.arange(5)], [0])),
    "fdrand_5x4x3": lambda esp: esp.fdrand(5, 4, 3),
    "fdrand_9x7x1": lambda esp: esp.fdrand(9, 7, 1),
    "fdrand_30x1x1": lambda esp: esp.fdrand(30, 1, 1),
    "convdiff_6x5x4": lambda esp: convdiff(esp, 6, 5, 4, 4.0),
    "lower_bidiagonal_2000": lambda esp: bidiagonal(esp, 2000, True),
    "upper_bidiagonal_2000": lambda esp: bidiagonal(esp, 2000, False),
    "random_5000": lambda esp: random_nonsymmetric(esp, 5000),
    "arrow_long": lambda esp: arrow(esp, AMG_LONG),
    "arrow_long_plus_1": lambda esp: arrow(esp, AMG_LONG + 1),
    "arrow_65": lambda esp: arrow(esp, 65),
    "arrow_5000": lambda esp: arrow(esp, 5000),
    "dense_64": lambda esp: dense(esp, 64),
}


def check_structure(P, model, arrays):
    """colours, permutation, coloring() and A[c,c] against the model -> the model's Coloring"""
    col = model.coloring(arrays[0], arrays[1])
    assert P.ncolors == col.ncolors
    assert np.array_equal(P.colors(), col.color)
    assert np.array_equal(P.permutation(), col.c + 1)
    got = P.coloring()
    assert len(got) == col.ncolors and all(np.array_equal(a, b) for a, b in zip(got, col.lists()))
    cp, rv, nz = P.reordered_matrix()
    wcp, wrv, wnz = model.reorder(arrays, col.c)
    assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv) and np.array_equal(bits(nz), bits(wnz))
    return col


def check_numbers(P, BM, kind, model, arrays, col, seed=1):
    """ldiv (also with out is v, host and device vectors), and for ILUAM the factor and the level counts"""
    import torch
    v = np.random.default_rng(seed).standard_normal(BM.n)
    want = BM.ldiv(v)
    assert same_bits(P.ldiv(v), want)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, want)
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), want)
    if kind == "iluam":
        assert same_bits(P.factor(), BM.factor(True))
        bcp, brv, _ = model.reorder(arrays, col.c)
        assert P.levels() == tuple(int(lev.max()) + 1 for lev in level_schedules(bcp, brv))
        assert max(P.levels()) <= col.ncolors
    return want


def check_all(esp, orc, model, bmodel, A, kind):
    arrays = host_arrays(A)
    P = esp.ColoredPreconditioner(A, factorization(esp, kind))
    try:
        col = check_structure(P, model, arrays)
        BM = colored_model(bmodel, orc, kind, arrays, col.c)
        check_numbers(P, BM, kind, model, arrays, col)
        return col
    finally:
        P.close()


# ---- the shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes(esp, orc, model, bmodel, kind, shape):
    A = SHAPES[shape](esp)
    col = check_all(esp, orc, model, bmodel, A, kind)
    n = A.n
    if shape == "diagonal5":
        assert col.ncolors == 1 and np.array_equal(col.c, np.arange(n))
    if shape == "dense_64":
        assert col.ncolors == 64
    if shape == "random_5000":
        assert col.ncolors > 3 and n > 4 * 256 and col.ptr[1] < n // 2      # several workgroups, and the lists shrink
    if shape.startswith("arrow"):
        cp = host_arrays(A)[0]
        assert cp[1] - cp[0] == n and (n > AMG_LONG) == (shape != "arrow_long")


@pytest.mark.parametrize("kind", KINDS)
def test_empty_matrix(esp, kind):
    A = esp.ExtendableSparseMatrix(0, 0)
    P = esp.ColoredPreconditioner(A, factorization(esp, kind))
    assert P.ncolors == 0 and len(P.colors()) == 0 and len(P.permutation()) == 0 and P.coloring() == []
    assert len(P.ldiv(np.zeros(0))) == 0
    x, log = esp.cg(A, np.zeros(0), Pl=P, log=True)
    assert log["iters"] == 0 and log["isconverged"]
    assert esp.graphcol(A) == []
    P.update()
    P.close()


# ---- reproducibility and updates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_and_values_only_update(esp, orc, model, bmodel, kind):
    A = esp.fdrand(9, 7, 3)
    n = A.n
    P = esp.ColoredPreconditioner(A, factorization(esp, kind))
    Q = esp.ColoredPreconditioner(A, factorization(esp, kind))
    assert np.array_equal(P.colors(), Q.colors()) and np.array_equal(P.permutation(), Q.permutation())
    Q.close()
    colors, perm = P.colors(), P.permutation()
    v = np.random.default_rng(6).standard_normal(n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: A[c,c] holds copies, for ILU0 too
    P.update()
    arrays = host_arrays(A)
    assert np.array_equal(P.colors(), colors) and np.array_equal(P.permutation(), perm)
    col = check_structure(P, model, arrays)
    u_new = check_numbers(P, colored_model(bmodel, orc, kind, arrays, col.c), kind, model, arrays, col, seed=6)
    assert not same_bits(u_new, u_old)
    F = esp.ColoredPreconditioner(A, factorization(esp, kind))
    assert same_bits(F.ldiv(v), u_new)
    cp, rv, nz = P.reordered_matrix()
    fcp, frv, fnz = F.reordered_matrix()
    assert np.array_equal(cp, fcp) and np.array_equal(rv, frv) and np.array_equal(bits(nz), bits(fnz))
    if kind == "iluam":
        assert same_bits(P.factor(), F.factor()) and P.levels() == F.levels()
    F.close()
    P.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pattern_change_needs_update_and_recolours(esp, orc, model, bmodel, kind):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    P = esp.ColoredPreconditioner(A, factorization(esp, kind))
    before = P.colors()
    v = np.random.default_rng(6).standard_normal(n)
    i, j = 1, n                                           # a new coupling between two unknowns of one colour, if there is one
    same = np.flatnonzero(before == before[0])
    if len(same) > 1:
        i, j = int(same[0]) + 1, int(same[-1]) + 1
    A.append(esp.ESP_UPDATE, [i], [j], [0.125])
    A.flush()
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    with pytest.raises(esp.EspError) as e:
        esp.gmres(A, v, Pl=P)
    assert e.value.code == ESP_ERR_STATE
    with pytest.raises(esp.EspError) as e:
        P.colors()
    assert e.value.code == ESP_ERR_STATE
    P.update()
    arrays = host_arrays(A)
    assert len(arrays[1]) == len(P.reordered_matrix()[1])
    col = check_structure(P, model, arrays)
    assert col.color[i - 1] != col.color[j - 1] and not np.array_equal(col.color, before)
    check_numbers(P, colored_model(bmodel, orc, kind, arrays, col.c), kind, model, arrays, col, seed=6)
    P.close()


# ---- levels -----------------------------------------------------------------------------------------------------------------------
def test_levels_collapse_on_fdrand_20_cubed(esp):
    A = esp.fdrand(20, 20, 20)
    P = esp.ColoredPreconditioner(A, esp.ILUAMPreconditioner)
    U = esp.ILUAMPreconditioner(A)
    print("fdrand 20^3: %d colours, levels coloured %s, natural %s" % (P.ncolors, P.levels(), U.levels()))
    assert max(P.levels()) <= P.ncolors
    assert all(a < b for a, b in zip(P.levels(), U.levels())) and P.ncolors < min(U.levels())
    P.close()
    U.close()


# ---- the shared builder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_block_preconditioner_over_the_permutation(esp, kind):
    A = convdiff(esp, 6, 5, 4, 4.0)
    P = esp.ColoredPreconditioner(A, factorization(esp, kind))
    Q = esp.BlockPreconditioner(A, [P.permutation()], factorization(esp, kind))
    assert Q.path == 1
    v = np.random.default_rng(3).standard_normal(A.n)
    assert same_bits(P.ldiv(v), Q.ldiv(v))
    for a, b in zip(P.reordered_matrix(), Q.block_matrix()):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    if kind == "iluam":
        assert same_bits(P.factor(), Q.factor()) and P.levels() == Q.levels()
    P.close()
    Q.close()


def test_graph_coloring_call(esp, model):
    import torch
    A = random_nonsymmetric(esp, 700, seed=2)
    P = esp.ParallelILU0Preconditioner(A)
    got = esp.graphcol(A)
    assert len(got) == P.ncolors and all(np.array_equal(a, b) for a, b in zip(got, P.coloring()))
    arrays = host_arrays(A)
    col = model.coloring(arrays[0], arrays[1])
    lib, h = A._d.lib, A._d.h
    nc = C.c_int64()
    t = torch.full((A.n,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.esp_graph_coloring(h, C.byref(nc), C.c_void_p(t.data_ptr()), 1) == 0
    assert nc.value == col.ncolors and np.array_equal(t.cpu().numpy(), col.color)
    nc2 = C.c_int64()
    assert lib.esp_graph_coloring(h, C.byref(nc2), None, 0) == 0 and nc2.value == col.ncolors       # the count alone
    d = torch.empty(A.n, dtype=torch.int64, device="cuda")
    assert lib.esp_precon_colored_perm(P._p, C.c_void_p(d.data_ptr()), 1) == 0
    assert np.array_equal(d.cpu().numpy(), col.c)
    assert lib.esp_precon_colored_colors(P._p, C.c_void_p(d.data_ptr()), 1) == 0
    assert np.array_equal(d.cpu().numpy(), col.color)
    out = (C.c_int64 * 2)()
    assert lib.esp_precon_colored_info(P._p, out) == 0 and (out[0], out[1]) == (col.ncolors, len(arrays[1]))
    P.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, kind):
    p = C.c_void_p()
    rc = lib.esp_precon_colored_create(h, kind, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    lib, h = A._d.lib, A._d.h
    for kind in (-1, 0, 3, 4, 5, 6, 7):                  # Jacobi, Block, AMG, ILU(k) and the kind itself are no inner kinds
        assert raw_create(lib, h, kind)[0] == ESP_ERR_INVALID
    rc, p, _ = raw_create(lib, h, 1)
    assert rc == 0
    assert lib.esp_destroy(h) == ESP_ERR_STATE            # refused while p lives
    out = (C.c_int64 * 2)()
    b = C.c_void_p()
    Q = esp.ILU0Preconditioner(A)                         # the inspectors refuse another kind
    assert lib.esp_precon_colored_info(Q._p, out) == ESP_ERR_INVALID
    assert lib.esp_precon_colored_matrix(Q._p, C.byref(b)) == ESP_ERR_INVALID
    assert lib.esp_precon_block_matrix(p, C.byref(b), None) == ESP_ERR_INVALID
    Q.close()
    assert lib.esp_precon_destroy(p) == 0
    # pending entries (appended through the C call, which does not flush)
    one = np.ones(1, np.int64)
    val = np.ones(1)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h, 1)[0] == ESP_ERR_STATE
    nc = C.c_int64()
    assert lib.esp_graph_coloring(h, C.byref(nc), None, 0) == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # a rectangular matrix
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h, 1)[0] == ESP_ERR_INVALID
    assert lib.esp_graph_coloring(R._d.h, C.byref(nc), None, 0) == ESP_ERR_INVALID
    # a column without a stored diagonal
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 2.0]])))
    for kind in (1, 2):
        rc, _, msg = raw_create(M._d.lib, M._d.h, kind)
        assert rc == ESP_ERR_INVALID and "diagonal" in msg
    assert lib.esp_graph_coloring(M._d.h, C.byref(nc), None, 0) == 0 and nc.value in (2, 3)      # the colouring itself needs none
    with pytest.raises(TypeError):
        esp.ColoredPreconditioner(A, esp.JacobiPreconditioner)
    with pytest.raises(TypeError):
        esp.ColoredPreconditioner(A, "ilu0")


def test_column_window_is_unsupported(esp):
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.ColoredPreconditioner(A, esp.ILU0Preconditioner)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                          # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    for kind in (1, 2):
        rc, _, msg = raw_create(lib, h, kind)
        assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    nc = C.c_int64()
    assert lib.esp_graph_coloring(h, C.byref(nc), None, 0) == ESP_ERR_UNSUPPORTED
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, v.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_STATE
    P.close()


def test_create_destroy_loop_does_not_leak(esp):
    """the device's free memory, read through the runtime, must not keep falling over 20 create / update / destroy cycles"""
    import torch
    A = esp.fdrand(20, 20, 20)

    def cycle(k):
        for _ in range(k):
            for fact in (esp.ILU0Preconditioner, esp.ILUAMPreconditioner):
                P = esp.ColoredPreconditioner(A, fact)
                P.update()
                P.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle(2)
    free0 = cycle(1)
    free1 = cycle(20)
    assert free0 - free1 < (8 << 20), (free0, free1)      # A[c,c] and its factorization at 20^3 hold a few MiB


# ---- solvers ------------------------------------------------------------------------------------------------------------------------
SOLVER = {}


def solver_matrix(esp, bmodel, name):
    if name not in SOLVER:
        A = esp.fdrand(12, 10, 8) if name == "fdrand" else convdiff(esp, 12, 10, 8, 4.0)
        arrays = host_arrays(A)
        SOLVER[name] = (A, arrays, bmodel.mul(arrays, np.ones(A.n)))
    return SOLVER[name]


def solver_model(esp, orc, model, bmodel, name, kind):
    """(A, b, the preconditioner, its model), the models shared by the tests of one matrix and kind"""
    A, arrays, b = solver_matrix(esp, bmodel, name)
    if (name, kind) not in SOLVER:
        col = model.coloring(arrays[0], arrays[1])
        SOLVER[(name, kind)] = colored_model(bmodel, orc, kind, arrays, col.c)
    return A, b, esp.ColoredPreconditioner(A, factorization(esp, kind)), SOLVER[(name, kind)]


def to_device(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def to_host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_simple(esp, orc, model, bmodel, kind, where):
    A, b, P, BM = solver_model(esp, orc, model, bmodel, "fdrand", kind)
    u0 = np.random.default_rng(12).standard_normal(A.n)
    uu = u0.copy() if where == "host" else to_device(u0)
    got, log = esp.simple(A, b if where == "host" else to_device(b), u=uu, Pl=P, maxiter=5, reltol=0.0, log=True)
    wu, wh, wit = BM.simple(b, u=u0, maxiter=5, reltol=0.0)
    assert wit == 5 and len(log["resnorm"]) == 6
    assert same_bits(to_host(got), wu) and same_bits(log["resnorm"], wh)
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg(esp, orc, model, bmodel, kind, where):
    A, b, P, BM = solver_model(esp, orc, model, bmodel, "fdrand", kind)
    for kw in ({"maxiter": 8}, {}):
        x, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, log=True, **kw)
        wx, wh, wit, wconv = BM.cg(b, **kw)
        assert log["iters"] == wit and log["isconverged"] == wconv
        assert same_bits(history_of(log), wh) and same_bits(to_host(x), wx)
    assert log["isconverged"] and np.linalg.norm(to_host(x) - 1.0) <= 1e-6 * np.sqrt(A.n)
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_bicgstabl(esp, orc, model, bmodel, kind, where):
    A, b, P, BM = solver_model(esp, orc, model, bmodel, "convdiff", kind)
    for kw in ({"max_mv_products": 12}, {}):
        x, log = esp.bicgstabl(A, b if where == "host" else to_device(b), l=2, Pl=P, log=True, **kw)
        wx, wh, wit, wmv, wconv = BM.bicgstabl(b, l=2, **kw)
        assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv)
        assert same_bits(history_of(log), wh) and same_bits(to_host(x), wx)
    assert log["isconverged"]
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "torch"])
def test_gmres(esp, orc, model, bmodel, gmodel, kind, where):
    A, b, P, BM = solver_model(esp, orc, model, bmodel, "convdiff", kind)
    for kw in ({"maxiter": 7}, {}):
        x, log = esp.gmres(A, b if where == "host" else to_device(b), Pl=P, restart=20, log=True, **kw)
        want = gmodel.gmres_cb(BM, A.n, b, restart=20, **kw)
        assert (log["iters"], log["mvps"], log["reorth"], log["isconverged"]) == (want.iters, want.mvps, want.reorth, want.converged)
        assert same_bits(history_of(log), want.history) and same_bits(to_host(x), want.x)
    assert log["isconverged"]
    P.close()


# ---- the reference's acceptance test ---------------------------------------------------------------------------------------------------
# seeds chosen on the CPU with the model pair (NOTES/coloring.md): both model runs converge in the same number of iterations
REPLAY = {10: 32, 100: 31, 1000: 31}


@pytest.mark.parametrize("n", sorted(REPLAY))
def test_replay_of_test_parilu0(esp, orc, model, bmodel, gmodel, n):
    """test/test_parilu0.jl: gmres(A, b, Pl = ParallelILU0Preconditioner(A)) against gmres(A_r, b_r, Pl = ILU0Preconditioner(A_r)) with
    A_r, b_r = reorderlinsys(A, b, coloring): equal iteration counts and x_par[c] ~ x_ser.  The two runs add their dot products in
    different orders; the tolerance is 16 times the difference the model pair shows for the seed."""
    csc = dominant_nonsymmetric(n, REPLAY[n])
    col = model.coloring(csc[0], csc[1])
    par, ser, b = replay_pair(gmodel, bmodel, orc, csc, col)
    diff = float(np.max(np.abs(par.x[col.c] - ser.x)))
    assert par.converged and ser.converged and par.iters == ser.iters and diff > 0.0          # the model pair satisfies both conditions
    A = from_arrays(esp, *csc)
    P = esp.ParallelILU0Preconditioner(A)
    coloring = P.coloring()
    assert all(np.array_equal(a, w) for a, w in zip(coloring, col.lists())) and len(coloring) == col.ncolors
    x_par, log_par = esp.gmres(A, b, Pl=P, log=True)
    A_r, b_r = esp.reorderlinsys(A, b, coloring)
    for a, w in zip(host_arrays(A_r), model.reorder(csc, col.c)):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(w) if w.dtype == np.float64 else w)
    assert same_bits(b_r, b[col.c])
    S = esp.ILU0Preconditioner(A_r)
    x_ser, log_ser = esp.gmres(A_r, b_r, Pl=S, log=True)
    got = float(np.max(np.abs(x_par[col.c] - x_ser)))
    print("replay n = %d seed %d: %d colours, iterations %d / %d, |x_par[c] - x_ser| device %.3e, model %.3e"
          % (n, REPLAY[n], col.ncolors, log_par["iters"], log_ser["iters"], got, diff))
    assert log_par["isconverged"] and log_ser["isconverged"]
    assert log_par["iters"] == log_ser["iters"] == par.iters
    assert got <= 16.0 * diff
    assert np.max(np.abs(x_ser - 1.0)) <= 1e-6
    P.close()
    S.close()
