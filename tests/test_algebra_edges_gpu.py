"""GPU: the algebra, transpose and set-up kernels exactly at their compile-time edges (tests/algebra_patterns.py builds the
patterns, tests/test_edge_patterns.py checks on the CPU that they are what they claim): the shared column sorts at 8|9, 16|17, 32|33
and 4096|4097 -- through the transpose and, with descending and shuffled input, through BlockPreconditioner --, the wave compaction
of block.hip at 32|33, the 2048-entry tiles of the entry-parallel kernels, the 1024-element tiles of A+-B, the whole-wave columns of
transpose(A)*x and of the AMG restriction at 64|65, the dense coarse inverse up to 512, the reduction grids of norm and opnorm, and
the lane | workgroup expansion of ILU(k)'s search at 16|17.  Every comparison is against the C models the suite has, on bits; the
one exception is the run-to-run reproducibility of the norms."""
import ctypes as C

import numpy as np
import pytest

import algebra_patterns as ap
import amg_modellib as am
import block_precon_modellib
import iluk_modellib
import linalg_modellib
import matops_modellib
import rsamg_modellib as rs
import test_amg_gpu
import test_block_precon_gpu as tb
import test_iluk_gpu
import test_rsamg_gpu
from linalg_modellib import norm_exact, norm_ref
from matops_modellib import OP_ADD, OP_SUB
from refmodel import bits
from test_linalg_gpu import INF, NORM_P, assert_raw, check_mul_transpose, check_transpose, close, same_bits
from test_matops_gpu import arrays, assert_same, ext

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID = -1


@pytest.fixture(scope="module")
def linalg(tmp_path_factory):
    return linalg_modellib.Model(tmp_path_factory.mktemp("algebra_linalg_model"))


@pytest.fixture(scope="module")
def matops(tmp_path_factory):
    return matops_modellib.Model(tmp_path_factory.mktemp("algebra_matops_model"))


@pytest.fixture(scope="module")
def block_model(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("algebra_block_model"))


@pytest.fixture(scope="module")
def amg_model(tmp_path_factory):
    return am.Model(tmp_path_factory.mktemp("algebra_amg_model"))


@pytest.fixture(scope="module")
def rs_model(tmp_path_factory):
    return rs.Model(tmp_path_factory.mktemp("algebra_rsamg_model"))


@pytest.fixture(scope="module")
def iluk_model(tmp_path_factory):
    return iluk_modellib.Model(tmp_path_factory.mktemp("algebra_iluk_model"))


def last_transpose(T):
    """esp_debug_last_transpose of a result: (path taken, columns listed for the workgroup sort, longest column)"""
    out = (C.c_int64 * 3)(-7, -7, -7)
    assert T._d.lib.esp_debug_last_transpose(T._d.h, out) == 0
    return tuple(int(v) for v in out)


# ---- the column sorts through the transpose -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", ap.SORT_MAXIMA)
def test_sorts_through_the_transpose(esp, linalg, mx):
    """C's column lengths are the prescribed ones, their maximum exactly mx: the template of that maximum is the one launched"""
    lengths = ap.sort_sublists()[mx]
    X = ap.prescribed_lengths(lengths, seed=mx)
    A = ext(esp, len(lengths), ap.transpose_csc(ap.SORT_ROWS, X))
    want = linalg.transpose(A.m, arrays(A))
    assert_raw(want, X, "the model's transpose of the transposed pattern")
    nlong = sum(l > ap.COLSORT_LANE for l in lengths)
    assert nlong == {32: 0, 33: 1}.get(mx, nlong)
    for path in (1, 2, 0):
        T = A.transpose(path=path)
        assert_raw(arrays(T), want, "transpose path %d" % path)
        took = last_transpose(T)
        if path == 1:
            assert took == (1, 0, 0)
        elif mx <= ap.COLSORT_BLOCK:
            assert took == (2, nlong, mx)
        else:
            assert took == (1, nlong, mx)            # a column of 4097: counted, then handed to the generic path
        assert_raw(arrays(T), want, "the inspection call changes nothing")


def test_last_transpose_before_any_transpose_and_on_an_empty_operand(esp):
    Z = esp.ExtendableSparseMatrix(30, 20)
    assert last_transpose(Z) == (0, 0, 0)
    assert last_transpose(Z.transpose()) == (0, 0, 0)
    out = (C.c_int64 * 3)()
    lib = Z._d.lib
    assert lib.esp_debug_last_transpose(None, out) == ESP_ERR_INVALID and lib.esp_debug_last_transpose(Z._d.h, None) == ESP_ERR_INVALID


# ---- the column sorts with worst-case input, through BlockPreconditioner ---------------------------------------------------------------
SQUARE = {}


def square(esp, mx):
    if mx not in SQUARE:
        lengths = [l for l in ap.sort_sublists()[mx] if l >= 1]
        csc, n, where = ap.prescribed_square(lengths, seed=mx)
        assert [int(np.diff(csc[0])[c]) for c in where] == lengths and max(lengths) == mx
        SQUARE[mx] = (csc, n)
    csc, n = SQUARE[mx]
    return ext(esp, n, csc), n


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
@pytest.mark.parametrize("order", ["reversed", "shuffled", "zigzag"])
@pytest.mark.parametrize("mx", ap.SORT_MAXIMA)
def test_sorts_with_worst_case_input(esp, orc, block_model, mx, order, kind):
    """one partition [n-1, ..., 0]: every column reaches its sort strictly descending; a shuffled partition; [evens descending,
    odds ascending]: a descending and an ascending run.  mx = 4097 leaves through the generic route"""
    A, n = square(esp, mx)
    parts = ap.worst_case_partitions(n)[order]
    u = tb.check_all(esp, orc, block_model, A, parts, kind)
    assert np.isfinite(u).all()


# ---- BK_LONG -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True])
def test_compaction_at_32_and_33(esp, force):
    csc, n, parts = ap.compaction_edges()
    A = ext(esp, n, csc)
    a = arrays(A)
    assert np.array_equal(bits(a[2]), bits(csc[2]))
    wcp = block_precon_modellib.block_matrix(a, parts, force)[0]
    if not force:
        assert [int(wcp[t + 1] - wcp[t]) for t in range(len(ap.BK_CASES))] == [k for _, k in ap.BK_CASES]
    P = tb.make(esp, A, parts, "jacobi", force)
    try:
        tb.check_b(P, a, parts, force)
    finally:
        P.close()


# ---- tile borders of the entry-parallel kernels --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bordered(esp):
    csc = ap.bordered()
    return csc


def test_bordered_transpose(esp, linalg, bordered):
    A = ext(esp, ap.BORDERED_ROWS, bordered)
    check_transpose(esp, linalg, A)
    per_row = np.bincount(bordered[1] - 1, minlength=ap.BORDERED_ROWS)
    assert last_transpose(A.transpose(path=2)) == (2, int(np.sum(per_row > ap.COLSORT_LANE)), int(per_row.max()))


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("side", ["left", "right"])
def test_bordered_diag_scale(esp, matops, bordered, side, inplace):
    m, n = ap.BORDERED_ROWS, len(bordered[0]) - 1
    d = np.random.default_rng(3).standard_normal(m if side == "left" else n)
    if side == "left":
        d[::7], d[3::11] = 0.0, -0.0
    else:
        d[6], d[35], d[8] = 0.0, -0.0, -1.5      # the column on the border, the last tile's only entry, the column of three tiles
    want = matops.diag_scale(bordered, d, 0 if side == "left" else 1)
    A = ext(esp, m, bordered)
    if inplace:
        R = A.diag_scale(d, side=side, inplace=True)
        assert R is A
    else:
        R = esp.Diagonal(d) * A if side == "left" else A * esp.Diagonal(d)
        assert_raw(arrays(A), bordered, "the operand")
    assert_same(arrays(R), want, "diag scale " + side)


def test_bordered_mul_transpose(esp, linalg, bordered):
    A = ext(esp, ap.BORDERED_ROWS, bordered)
    check_mul_transpose(esp, linalg, A, np.random.default_rng(4).standard_normal(ap.BORDERED_ROWS))


def test_issymmetric_at_the_tile_borders(esp, linalg):
    csc = ap.symmetric_bordered()
    n = ap.SYM_N

    def sym(c):
        got = ext(esp, n, c).issymmetric()
        assert got == linalg.issymmetric(n, c)
        return got
    assert sym(csc)
    for p in ap.SYM_POSITIONS + [len(csc[1]) - 1]:
        assert not sym(ap.perturbed(csc, p)), p                   # the only asymmetric value is the first / last entry of a tile
        assert sym(ap.zero_pair(csc, p)), p                       # +0.0 against -0.0


# ---- A+B, A-B --------------------------------------------------------------------------------------------------------------------------
MERGE = {}


def merge_case(name):
    if not MERGE:
        MERGE.update(ap.merge_cases())
    return MERGE[name]


MERGE_NAMES = ["split", "split_cancel", "a_exhausted", "b_exhausted", "a_empty", "b_empty", "tile_cancels_add", "tile_cancels_sub",
               "columns_cancel_add", "columns_cancel_sub", "total1024", "total1025", "total2048", "total2049", "column_border"]


def test_merge_names():
    assert sorted(MERGE_NAMES) == sorted(ap.merge_cases())


@pytest.mark.parametrize("op", ["+", "-"])
@pytest.mark.parametrize("name", MERGE_NAMES)
def test_merge_path(esp, matops, name, op):
    c = merge_case(name)
    A, B, m = c["A"], c["B"], c["m"]
    Ae, Be = ext(esp, m, A), ext(esp, m, B)
    want = matops.add(A, B, OP_ADD if op == "+" else OP_SUB)
    R = Ae + Be if op == "+" else Ae - Be
    got = arrays(R)
    assert_same(got, want, "%s: A%sB" % (name, op))
    assert R.nnz() == len(want[1]) == sum(ap.kept_per_tile(A, B, op == "-"))
    for j in c.get("empty_columns", {}).get(op, []):
        assert got[0][j + 1] == got[0][j], j
    assert_raw(arrays(Ae), A, "operand A")
    assert_raw(arrays(Be), B, "operand B")


@pytest.mark.parametrize("name", [n for n in MERGE_NAMES if n != "a_empty"])
def test_merge_path_aliased(esp, matops, name):
    """A + A and A - A: both operands one handle; every pair lies inside its tile or is split by a border (an odd tile start)"""
    c = merge_case(name)
    A, m = c["A"], c["m"]
    Ae = ext(esp, m, A)
    assert_same(arrays(Ae + Ae), matops.add(A, A, OP_ADD), name + ": A+A")
    D = Ae - Ae
    got = arrays(D)
    assert_same(got, matops.add(A, A, OP_SUB), name + ": A-A")
    assert D.nnz() == 0 and np.all(got[0] == 1)


# ---- whole-wave columns of transpose(A)*x ---------------------------------------------------------------------------------------------
def test_wave_columns(esp, linalg):
    csc, lengths = ap.wave_columns()
    A = ext(esp, ap.WAVE_M, csc)
    want = check_mul_transpose(esp, linalg, A, ap.wave_x())          # host and device vectors
    assert np.isnan(want).any() and np.isfinite(want).any()
    check_mul_transpose(esp, linalg, A, np.random.default_rng(7).standard_normal(ap.WAVE_M))
    check_transpose(esp, linalg, A)


# ---- AMG and RS-AMG --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [31, 32, 63, 64])
def test_star_ldiv(esp, amg_model, rs_model, deg):
    """the hub column of A holds deg + 1 entries (32 | 33: AMG_LONG), the prolongation's only column as many (64 | 65: the
    restriction's AMG_TLONG)"""
    csc = am.star_graph(deg, hub=deg // 2)
    M = test_amg_gpu.check_all(esp, amg_model, csc, max_coarse=1)
    assert [L.n for L in M.levels] == [deg + 1, 1] and len(M.levels[0].P[1]) == deg + 1
    M = test_rsamg_gpu.check_all(esp, rs_model, csc, max_coarse=1)
    assert M.levels[0].n == deg + 1 and M.levels[-1].n == 1


DENSE_SIZES = [127, 128, 129, 511, 512]


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_coarse_inverse_direct(esp, amg_model, n):
    a = np.random.default_rng(n).standard_normal((n, n)) + n * np.eye(n)
    M = test_amg_gpu.check_all(esp, amg_model, test_amg_gpu.full_csc(a), max_levels=1, max_coarse=1)
    assert len(M.levels) == 1 and M.inv.shape == (n, n)
    assert np.abs(M.inv @ a - np.eye(n)).max() < 1e-12


def path_with_aggregates(model, n):
    """the smallest path whose first aggregation leaves exactly n unknowns"""
    for size in range(2 * n, 6 * n):
        g = am.path_graph(size)
        if model.aggregate(g, model.strength(g, 0.0))[1] == n:
            return size
    raise AssertionError(n)


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_coarse_inverse_below_a_fine_level(esp, amg_model, n):
    size = path_with_aggregates(amg_model, n)
    M = test_amg_gpu.check_all(esp, amg_model, am.path_graph(size), max_coarse=n)
    assert [L.n for L in M.levels] == [size, n] and M.inv.shape == (n, n) and np.isfinite(M.inv).all()


def test_coarse_inverse_row_swaps_and_zero_pivot_at_512(esp, amg_model):
    """170 copies of the 3 x 3 matrix with a stored zero diagonal and |4| == |-4| (a row swap in every block, the first of two equal
    pivots taken) and a 2 x 2 block: n = 512; and 256 singular 2 x 2 blocks: a zero pivot is no error"""
    swap = np.array([[0.0, 2.0, 1.0], [4.0, 1.0, 0.0], [-4.0, 3.0, 5.0]])
    a = np.zeros((512, 512))
    a[:510, :510] = np.kron(np.eye(170), swap)
    a[510:, 510:] = [[3.0, 1.0], [1.0, 2.0]]
    M = test_amg_gpu.check_all(esp, amg_model, test_amg_gpu.full_csc(a), max_levels=1)
    assert np.abs(M.inv @ a - np.eye(512)).max() < 1e-13
    z = np.kron(np.eye(256), np.array([[1.0, 2.0], [2.0, 4.0]]))
    M = test_amg_gpu.check_all(esp, amg_model, test_amg_gpu.full_csc(z), max_levels=1)
    assert not np.isfinite(M.inv).all()


def test_max_coarse_513_is_refused(esp):
    A = test_amg_gpu.matrix(esp, am.path_graph(5))
    for kind in (esp.AMGPreconditioner, esp.RS_AMGPreconditioner):
        with pytest.raises(esp.EspError) as e:
            kind(A, max_coarse=513)
        assert e.value.code == ESP_ERR_INVALID and "max_coarse = 513 (1..512" in str(e.value)
        kind(A, max_coarse=512).close()


# ---- the reduction grids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("N", ap.RED_SIZES)
def test_norm_reduction_grids(esp, N, negative):
    """an N x 1 matrix with a dense column.  The element a second (third) round reads, or the one behind the 256th partial, carries
    1e3 (1e-3): tests/test_edge_patterns.py shows that the reference without it misses the bound for the p of that sign"""
    v = ap.reduction_vector(N, negative)
    A = ext(esp, N, ap.column_vector_csc(v))
    assert A.shape == (N, 1) and A.nnz() == N
    for p in NORM_P:
        g = A.norm(p)
        assert same_bits(g, A.norm(p)), ("norm not reproducible", p)
        e = norm_exact(v, p)
        if e is not None:
            assert same_bits(g, e), ("norm", p, g, e)
        else:
            w = norm_ref(v, p)
            assert close(g, w), ("norm", p, g, w)
            if p in (1, 2):                                   # the one-column branches of opnorm are the same reductions
                assert same_bits(A.opnorm(p), g)
    assert same_bits(A.opnorm(INF), norm_exact(v, INF))


# ---- MAX_GRID --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(esp):
    csc, n = ap.grid_matrix()
    return ext(esp, n, csc), csc, n


def test_opnorm_beyond_the_grid(linalg, grid):
    A, csc, n = grid
    for p in (1, INF):
        g, w = A.opnorm(p), linalg.opnorm_general(n, csc, p)
        assert same_bits(g, w), (p, g, w)
    assert same_bits(A.opnorm(1), A.opnorm(1))


def test_transpose_beyond_the_grid(linalg, grid):
    A, csc, n = grid
    want = linalg.transpose(n, csc)
    assert want[0][n] - want[0][n - 1] == 33
    for path in (2, 1):
        T = A.transpose(path=path)
        assert_raw(arrays(T), want, "transpose path %d" % path)
        assert last_transpose(T) == ((2, 1, 33) if path == 2 else (1, 0, 0))
        del T


# ---- ILU(k) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["lower", "upper"])
@pytest.mark.parametrize("width", [16, 17])
def test_iluk_frontier_vertex(esp, iluk_model, width, which, K):
    """a frontier vertex of exactly 16 (a lane expands it) and 17 stored rows (the workgroup does), reached at depth 1 and 2"""
    csc, tcsc, r1, r2 = ap.frontier(width)
    A = test_iluk_gpu.from_arrays(esp, *(csc if which == "lower" else tcsc))
    st, want = test_iluk_gpu.check_all(esp, iluk_model, A, K)
    assert st["wide_lower"] == 0 and st["wide_upper"] == 0           # the wave form served every column
    assert st["max_level"] >= min(K, 2)                              # (the model's largest level: check_b)
    if K >= 1:
        assert st["nnz"] >= A.nnz() + width - 2


@pytest.mark.parametrize("n", [4096, 4097])
def test_iluk_comb_at_the_column_sort(esp, iluk_model, n):
    """column 1 of B holds exactly n entries: the workgroup sort's last size and the first one above it"""
    A = test_iluk_gpu.from_scipy(esp, test_iluk_gpu.comb(n))
    st, want = test_iluk_gpu.check_all(esp, iluk_model, A, 1)
    assert st["nnz"] == 3 * n - 2 and st["max_level"] == 1
    assert np.diff(want.B[0])[1] == n == np.diff(want.B[0]).max()
