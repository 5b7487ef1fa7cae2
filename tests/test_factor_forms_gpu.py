"""GPU: the factorization side at its edges, on the crafted patterns of tests/factor_patterns.py.
1. ILUAM's two forms of the column factorization (iluam.hip: FactorOp, a lane per column, and FactorWaveOp, a wave per column): the
   switch at nnz == 24 n read back through last_factor_form(), and lane form, wave form and tests/iluam_model.c held to each other on
   columns of 2047 / 2048 / 2049 rows (the staging capacity FW_ROWS), on one, two and three rounds of the lane stride, on searches
   that hit, miss inside column j and run beyond its last row, on thin launches whose waves take several members and wide launches
   with a ragged last workgroup; the launch lists of tests/edge_patterns.py under a forced wave form; special values; a values-only
   update!; the kinds that forward the hook to their inner ILUAM.
2. LUFactorization's wave loops (lu.hip): nbr_max with several long vertices in one wave, at lanes 0 and 63, in the ragged last wave,
   long by the row alone; lu_bfill_k with nodes of 63 / 64 / 65 vertices, alone and in another column's transposed list.
Every comparison is on bits; there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

import edge_patterns as ep
import factor_patterns as fp
import iluk_modellib
import lu_modellib
from iluam_modellib import level_schedules
from refmodel import bits
from test_lu_gpu import check_all

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID = -1
LANE, WAVE = 1, 2


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    """lu_model.c; .iluam is iluam_model.c's Model"""
    return lu_modellib.Model(tmp_path_factory.mktemp("forms_lu_model"))


@pytest.fixture(scope="module")
def ik(tmp_path_factory):
    return iluk_modellib.Model(tmp_path_factory.mktemp("forms_iluk_model"))


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def finite_and_same(got, want):
    want = np.asarray(want, np.float64)
    return bool(np.isfinite(want).all()) and same_bits(got, want)


def from_arrays(esp, arrays):
    """a matrix with exactly the stored entries of the CSC arrays (explicit zeros and NaN included)"""
    cp, rv, nz = arrays
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(len(cp) - 1, len(cp) - 1, cp, rv, nz))


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def matrix_of(esp, case):
    """(A, its CSC arrays) of a factor_patterns case; the device holds the arrays the model reads"""
    I, J, V, n = case
    arrays = ep.csc_arrays(n, I, J, V)
    A = from_arrays(esp, arrays)
    got = host_arrays(A)
    assert np.array_equal(got[0], arrays[0]) and np.array_equal(got[1], arrays[1]) and same_bits(got[2], arrays[2])
    return A, arrays


def automatic_form(arrays):
    """iluam_update's rule on the arrays of the factored matrix"""
    return WAVE if len(arrays[1]) >= fp.FW_MIN_AVG * (len(arrays[0]) - 1) else LANE


def rule(cp, rv):
    """(levels, launches) of the three schedules of a pattern: level_schedules and the launch rule applied to its widths"""
    sched = level_schedules(cp, rv)
    return tuple(int(l.max()) + 1 for l in sched), tuple(ep.launch_list(ep.widths_of(l)) for l in sched)


def forced(P, form):
    P.debug_factor_form(form)
    P.update()
    return P.last_factor_form()


# =================================================================================================================================
# form selection
# =================================================================================================================================
@pytest.mark.parametrize("nnz,form", [(2400, WAVE), (2399, LANE)])
def test_switch_at_24_entries_per_column(esp, lm, nnz, form):
    """nnz == 24 n is the wave form, one entry less the lane form; both the model's bits; forcing overrides and 0 restores the rule"""
    A, arrays = matrix_of(esp, fp.exact_nnz(100, nnz, seed=5))
    assert A.nnz() == nnz and automatic_form(arrays) == form
    f, diag = lm.iluam.factor(arrays)
    P = esp.ILUAMPreconditioner(A)
    try:
        assert P.last_factor_form() == form
        assert finite_and_same(P.factor(), f)
        other = LANE + WAVE - form
        P.debug_factor_form(other)
        assert P.last_factor_form() == form                  # nothing ran yet
        P.update()
        assert P.last_factor_form() == other and finite_and_same(P.factor(), f)
        assert forced(P, 0) == form and finite_and_same(P.factor(), f)
        v = np.random.default_rng(1).standard_normal(A.n)
        assert finite_and_same(P.ldiv(v), lm.iluam.ldiv(arrays, f, diag, v))
    finally:
        P.close()


def test_no_factorization_reports_zero(esp):
    """n = 0, and ILUT's prefactored inner ILUAM whatever is forced"""
    E = esp.ExtendableSparseMatrix(0, 0)
    P = esp.ILUAMPreconditioner(E)
    assert P.last_factor_form() == 0 and forced(P, WAVE) == 0 and forced(P, LANE) == 0
    P.close()
    A = esp.fdrand(5, 4, 3)
    T = esp.ILUTPreconditioner(A)
    try:
        v = np.random.default_rng(1).standard_normal(A.n)
        u = T.ldiv(v)
        assert T.last_factor_form() == 0
        assert forced(T, WAVE) == 0 and same_bits(T.ldiv(v), u)
        assert forced(T, LANE) == 0 and same_bits(T.ldiv(v), u)
    finally:
        T.close()


def test_error_codes(esp):
    """both calls refuse the kinds without an (inner) ILUAM, a null preconditioner, a form outside 0..2 and a null result"""
    A = esp.fdrand(5, 4, 3)
    lib = A._d.lib
    form = C.c_int32(7)
    others = [esp.JacobiPreconditioner(A), esp.ILU0Preconditioner(A), esp.AMGPreconditioner(A), esp.RS_AMGPreconditioner(A),
              esp.SPAIPreconditioner(A), esp.SPAIPreconditioner(A, order=0), esp.ParallelILU0Preconditioner(A),
              esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.JacobiPreconditioner),
              esp.BlockPreconditioner(A, [range(1, A.n + 1)], esp.ILU0Preconditioner)]
    for P in others:
        for f in (0, 1, 2):
            assert lib.esp_debug_iluam_form(P._p, f) == ESP_ERR_INVALID, type(P).__name__
        assert lib.esp_debug_last_iluam_form(P._p, C.byref(form)) == ESP_ERR_INVALID and form.value == 7, type(P).__name__
        if hasattr(P, "debug_factor_form"):                   # (the classes that have .launches())
            with pytest.raises(esp.EspError) as e:
                P.debug_factor_form(1)
            assert e.value.code == ESP_ERR_INVALID
            with pytest.raises(esp.EspError):
                P.last_factor_form()
        P.close()
    assert lib.esp_debug_iluam_form(None, 1) == ESP_ERR_INVALID
    assert lib.esp_debug_last_iluam_form(None, C.byref(form)) == ESP_ERR_INVALID
    P = esp.ILUAMPreconditioner(A)
    for f in (-1, 3, 2 ** 31 - 1):
        assert lib.esp_debug_iluam_form(P._p, f) == ESP_ERR_INVALID
    assert lib.esp_debug_last_iluam_form(P._p, None) == ESP_ERR_INVALID
    assert lib.esp_debug_last_iluam_form(P._p, C.byref(form)) == 0 and form.value == LANE    # 7 entries per column
    P.update()
    assert P.last_factor_form() == LANE                       # the refused calls forced nothing
    P.close()


# =================================================================================================================================
# lane form, wave form and model on one matrix
# =================================================================================================================================
THREE_WAY = {
    "arrowband2047": lambda: fp.arrowband(2047),
    "arrowband2048": lambda: fp.arrowband(2048),
    "arrowband2049": lambda: fp.arrowband(2049),
    "arrowband2047_t": lambda: fp.transposed(fp.arrowband(2047)),
    "arrowband2048_t": lambda: fp.transposed(fp.arrowband(2048)),
    "arrowband2049_t": lambda: fp.transposed(fp.arrowband(2049)),
    "arrowband2049_middle": lambda: fp.arrowband(2049, hub=1024),
    "clique64": lambda: fp.cliques(1, 64),
    "clique65": lambda: fp.cliques(1, 65),
    "clique66": lambda: fp.cliques(1, 66),
    "clique131": lambda: fp.cliques(1, 131),
    "sparse_dense_enough": lambda: fp.sparse_dense_enough(seed=3),
    "cliques5x25": lambda: fp.cliques(5, 25),
    "cliques258x25": lambda: fp.cliques(258, 25),
}


@pytest.mark.parametrize("name", list(THREE_WAY))
def test_lane_wave_and_model_agree(esp, lm, name):
    """created under the automatic rule (the wave form), then forced to the lane form and back: the read-out follows, no bit of
    the factor moves, the launch list stays, and ldiv! is the model's"""
    A, arrays = matrix_of(esp, THREE_WAY[name]())
    assert automatic_form(arrays) == WAVE
    f, diag = lm.iluam.factor(arrays)
    P = esp.ILUAMPreconditioner(A)
    try:
        assert P.last_factor_form() == WAVE
        launches = P.launches()
        assert (P.levels(), launches) == rule(arrays[0], arrays[1])
        assert finite_and_same(P.factor(), f)
        assert forced(P, LANE) == LANE
        assert finite_and_same(P.factor(), f) and P.launches() == launches
        assert forced(P, WAVE) == WAVE
        assert finite_and_same(P.factor(), f) and P.launches() == launches
        v = np.random.default_rng(1).standard_normal(A.n)
        assert finite_and_same(P.ldiv(v), lm.iluam.ldiv(arrays, f, diag, v))
    finally:
        P.close()


# =================================================================================================================================
# the launch list under the wave form
# =================================================================================================================================
@pytest.mark.parametrize("name,form", [(name, form) for name in ep.WIDTHS for form in ("upper", "symmetric")])
def test_layered_launch_list_under_a_forced_wave_form(esp, lm, name, form):
    """3-5 entries per column: the lane form by the rule; forced, the wave kernels run the same launch list (thin folds, wide levels
    with a ragged last workgroup, thin groups between wide launches) to the model's bits"""
    I, J, V, n = ep.layered(ep.WIDTHS[name], form, seed=3)
    A, arrays = matrix_of(esp, (I, J, V, n))
    assert automatic_form(arrays) == LANE
    levels, launches = rule(arrays[0], arrays[1])
    assert launches[0] == ep.launch_list(ep.WIDTHS[name])
    f, diag = lm.iluam.factor(arrays)
    P = esp.ILUAMPreconditioner(A)
    try:
        assert P.last_factor_form() == LANE and (P.levels(), P.launches()) == (levels, launches)
        assert finite_and_same(P.factor(), f)
        assert forced(P, WAVE) == WAVE
        assert (P.levels(), P.launches()) == (levels, launches)
        assert finite_and_same(P.factor(), f)
        v = np.random.default_rng(1).standard_normal(n)
        assert finite_and_same(P.ldiv(v), lm.iluam.ldiv(arrays, f, diag, v))
    finally:
        P.close()


@pytest.mark.parametrize("copies", [256, 257, 258, 259, 260])
def test_clique_levels_of_256_to_260_columns(esp, lm, copies):
    """25 levels of `copies` columns under the automatic rule: a thin launch per level with 64 members per wave (256), wide launches
    whose last workgroup has 1, 2, 3, 4 live waves"""
    A, arrays = matrix_of(esp, fp.cliques(copies, 25))
    levels, launches = rule(arrays[0], arrays[1])
    assert launches[0] == ((0, 25) if copies == 256 else (25, 0))
    f, diag = lm.iluam.factor(arrays)
    P = esp.ILUAMPreconditioner(A)
    try:
        assert P.last_factor_form() == WAVE
        assert (P.levels(), P.launches()) == (levels, launches)
        assert finite_and_same(P.factor(), f)
    finally:
        P.close()


# =================================================================================================================================
# special values, a values-only update
# =================================================================================================================================
def special_cases():
    """cliques(3, 25) with a stored 0.0, -0.0 and NaN off-diagonal (one per block: the first block stays finite but for its own);
    and one whose pivots vanish: the first diagonal of block 1 is 0.0, and in block 2 a[1,1] = a[0,1] * (a[1,0] / a[0,0]) rounded,
    so the pivot of its column 1 is exactly 0.0 -- unless the update were contracted into a fused multiply-add"""
    I, J, V, n = fp.cliques(3, 25)
    cp, rv, nz = ep.csc_arrays(n, I, J, V)
    at = {(int(rv[q]) - 1, j): q for j in range(n) for q in range(cp[j] - 1, cp[j + 1] - 1)}
    a = nz.copy()
    a[at[(7, 3)]], a[at[(25 + 2, 25 + 9)]], a[at[(50 + 11, 50 + 4)]] = 0.0, -0.0, np.nan
    b = nz.copy()
    b[at[(25, 25)]] = 0.0
    b[at[(51, 51)]] = b[at[(50, 51)]] * (b[at[(51, 50)]] / b[at[(50, 50)]])
    return {"zeros_and_nan": (cp, rv, a), "zero_pivots": (cp, rv, b)}


@pytest.mark.parametrize("which", ["zeros_and_nan", "zero_pivots"])
def test_special_values_in_both_forms(esp, lm, which):
    arrays = special_cases()[which]
    f, diag = lm.iluam.factor(arrays)
    cp = arrays[0]
    blocks = [f[cp[25 * b] - 1:cp[25 * (b + 1)] - 1] for b in range(3)]
    if which == "zeros_and_nan":
        assert np.isfinite(blocks[0]).all() and np.isfinite(blocks[1]).all() and np.isnan(blocks[2]).any()
        zeros = arrays[2][arrays[2] == 0.0]
        assert len(zeros) == 2 and np.signbit(zeros).sum() == 1 and np.isnan(arrays[2]).sum() == 1
    else:
        assert np.isfinite(blocks[0]).all() and not np.isfinite(blocks[1]).all() and not np.isfinite(blocks[2]).all()
        assert f[cp[51] - 1 + 1] == 0.0                        # the pivot of column 1 of block 2: exactly zero
    A = from_arrays(esp, arrays)
    assert same_bits(host_arrays(A)[2], arrays[2]) and np.array_equal(np.signbit(host_arrays(A)[2]), np.signbit(arrays[2]))
    P = esp.ILUAMPreconditioner(A)
    try:
        assert P.last_factor_form() == WAVE and same_bits(P.factor(), f)
        assert forced(P, LANE) == LANE and same_bits(P.factor(), f)
        assert forced(P, WAVE) == WAVE and same_bits(P.factor(), f)
        v = np.random.default_rng(1).standard_normal(A.n)
        assert same_bits(P.ldiv(v), lm.iluam.ldiv(arrays, f, diag, v))
    finally:
        P.close()


def test_values_only_update_of_the_unstaged_column(esp, lm):
    """arrowband(2049) under the automatic rule: values changed in place, then update! -- bitwise a fresh create and the model"""
    A, arrays = matrix_of(esp, fp.arrowband(2049))
    cp, rv, nz0 = arrays
    f0, _ = lm.iluam.factor(arrays)
    P = esp.ILUAMPreconditioner(A)
    F = None
    try:
        launches = P.launches()
        csc = A.sparse()
        csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
        A._push_edits()
        cp1, rv1, nz1 = host_arrays(A)
        assert np.array_equal(cp1, cp) and np.array_equal(rv1, rv) and not np.array_equal(nz1, nz0)
        assert finite_and_same(P.factor(), f0)                 # no update!: the old factorization
        P.update()
        f1, diag = lm.iluam.factor((cp, rv, nz1))
        assert P.last_factor_form() == WAVE and P.launches() == launches
        assert finite_and_same(P.factor(), f1) and not same_bits(f1, f0)
        F = esp.ILUAMPreconditioner(A)
        assert same_bits(F.factor(), P.factor())
        v = np.random.default_rng(4).standard_normal(A.n)
        u = lm.iluam.ldiv((cp, rv, nz1), f1, diag, v)
        assert finite_and_same(P.ldiv(v), u) and same_bits(F.ldiv(v), u)
    finally:
        P.close()
        if F is not None:
            F.close()


# =================================================================================================================================
# the kinds that forward to their inner ILUAM
# =================================================================================================================================
def both_forms_through(P, B, fval, ldiv):
    """P: an outer preconditioner over the matrix B (host arrays); the read-out is the rule's on B, forcing the other form through
    P changes the read-out and no bit of factor() or ldiv!"""
    want = automatic_form(B)
    other = LANE + WAVE - want
    assert P.last_factor_form() == want
    assert same_bits(P.factor(), fval)
    v = np.random.default_rng(1).standard_normal(P.A.n)
    u = ldiv(v)
    assert same_bits(P.ldiv(v), u)
    launches = P.launches()
    for form in (other, want):
        assert forced(P, form) == form
        assert same_bits(P.factor(), fval) and same_bits(P.ldiv(v), u) and P.launches() == launches
    assert forced(P, 0) == want
    return want


def test_lu_forwards_the_form(esp, lm):
    A = esp.fdrand(5, 4, 3)
    want = lm.lu(host_arrays(A), 8)
    P = esp.LUFactorization(A, 8)
    try:
        form = both_forms_through(P, want.B, want.fval, want.ldiv)
        print("LU of fdrand(5, 4, 3), leaf_size 8: nnz(B) = %d, n = %d, form %d" % (len(want.B[1]), A.n, form))
    finally:
        P.close()


def test_iluk_forwards_the_form(esp, ik):
    A = esp.fdrand(5, 4, 3)
    want = ik.precon(host_arrays(A), 2)
    P = esp.ILUKPreconditioner(A, k=2)
    try:
        form = both_forms_through(P, want.B, want.fval, want.ldiv)
        print("ILU(2) of fdrand(5, 4, 3): nnz(B) = %d, n = %d, form %d" % (len(want.B[1]), A.n, form))
    finally:
        P.close()


def test_block_and_colored_forward_the_form(esp, lm):
    """on cliques(5, 25): one partition 1:n (B = A), and the multicolour reordering (B = A[c,c]); the inner read-out is the wave form"""
    A, arrays = matrix_of(esp, fp.cliques(5, 25))
    n = A.n
    f, diag = lm.iluam.factor(arrays)
    P = esp.BlockPreconditioner(A, [range(1, n + 1)], esp.ILUAMPreconditioner)
    try:
        assert P.path == 0
        assert both_forms_through(P, arrays, f, lambda v: lm.iluam.ldiv(arrays, f, diag, v)) == WAVE
    finally:
        P.close()
    Q = esp.ColoredPreconditioner(A)
    try:
        B = Q.reordered_matrix()
        fB, dB = lm.iluam.factor(B)
        c = Q.permutation() - 1

        def ldiv(v):
            out = np.empty(n)
            out[c] = lm.iluam.ldiv(B, fB, dB, np.ascontiguousarray(v[c]))
            return out
        assert both_forms_through(Q, B, fB, ldiv) == WAVE
    finally:
        Q.close()


# =================================================================================================================================
# LUFactorization's wave loops
# =================================================================================================================================
@pytest.mark.parametrize("hubs,entries,by", fp.MULTI_HUB_CASES)
def test_lu_with_several_long_vertices_in_a_wave(esp, lm, hubs, entries, by):
    """nbr_max folds every long vertex of a wave in turn: one at lane 0, at lane 63, both, two neighbours, three in one wave, one in
    the ragged last wave; long by the column (33), by the row alone (65), by both"""
    A, arrays = matrix_of(esp, fp.multi_hub(fp.MULTI_HUB_N, hubs, entries, by))
    bycol, byrow = fp.long_vertices(arrays[0], arrays[1])
    assert len(bycol) + len(byrow) >= len(hubs)
    check_all(esp, lm, A, 8)


@pytest.mark.parametrize("sizes,tail", [([63, 64, 65], 0), ([63, 64, 65], 10), fp.CLIQUE_TAILS_AT_THE_EDGE])
def test_lu_nodes_at_the_wave_edge(esp, lm, sizes, tail):
    """lu_bfill_k strides a node's rows 64 at a time: dense leaves of 63 / 64 / 65 vertices as components of their own, leaves of
    66 / 67 / 68 and of exactly 63 / 64 / 65 that a separator's column lists (tests/test_edge_patterns.py shows the sizes)"""
    A, arrays = matrix_of(esp, fp.clique_components(sizes, tail))
    st, want = check_all(esp, lm, A, 70)
    big = sorted(int(want.nsize[s]) for s in np.unique(want.nstart) if want.nsize[s] > 59)
    assert big == ([63, 64, 65] if tail in (0, 12) else [66, 67, 68]) and st["largest_node"] == big[-1]
