"""GPU: SPAIPreconditioner and ILUTPreconditioner at the edges of their compile-time capacities (NOTES/capacity_edges.md, "The
approximate-inverse and threshold side"), on the patterns of tests/approx_patterns.py, against tests/spai_model.c and
tests/ilut_model.c bit for bit: SPAI-1's workgroup tier up to its 12288 doubles and its sort up to 16384 words, both forms of the
size pass on either side of 512 and of 16384 rows, the q q rule, the grid-stride loops of both tiers, SPAI-0 over four lane strides,
and every end of the look-up branch of ILUT's sweep in its three tiers.  tests/test_edge_patterns.py shows on the CPU that the
patterns are what they claim."""
import numpy as np
import pytest

import approx_patterns as xp
import test_ilut_gpu as tig
import test_spai_gpu as tsg
from ilut_modellib import Model as IlutModel
from spai_modellib import Model as SpaiModel

pytestmark = pytest.mark.gpu

ESP_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def spai(tmp_path_factory):
    return SpaiModel(tmp_path_factory.mktemp("approx_spai_model"))


@pytest.fixture(scope="module")
def ilut(tmp_path_factory):
    return IlutModel(tmp_path_factory.mktemp("approx_ilut_model"))


def limits(esp):
    return esp._lib.ESP_SPAI_WAVE_DOUBLES, esp._lib.ESP_SPAI_DENSE_MAX


def expected_stats(esp, csc):
    """wide, max_p, max_q, max_pq by the rule restated on the arrays (every column is accepted)"""
    W, D = limits(esp)
    p, q, tc = xp.all_sizes(csc)
    assert (p * q).max() <= D and tc.max() <= xp.SORT_MAX
    wide = (q > 0) & ((p * q > W) | (q * q > W))
    return {"wide": int(wide.sum()), "max_p": int(p.max()), "max_q": int(q.max()), "max_pq": int((p * q).max())}


def set_values(A, nz):
    assert A._d.lib.esp_set_nzval(A._d.h, tsg.vp(np.ascontiguousarray(nz, np.float64))) == 0


def set_matrix(esp, A, csc):
    """a new stored matrix in the same handle: a pattern change of any kind"""
    cp, rv, nz = csc
    A.cscmatrix = esp.SparseMatrixCSC(len(cp) - 1, len(cp) - 1, cp.copy(), rv.copy(), nz.copy())


# ---- SPAI-1, accepted ----------------------------------------------------------------------------------------------------------------
ACCEPTED = {
    "block22": (lambda: xp.dense_block(22), {"wide": 0, "max_p": 22, "max_q": 22, "max_pq": 484}),
    "block23": (lambda: xp.dense_block(23), {"wide": 23, "max_p": 23, "max_q": 23, "max_pq": 529}),
    "block110": (lambda: xp.dense_block(110), {"wide": 110, "max_p": 110, "max_q": 110, "max_pq": 12100}),
    "full64x8": (lambda: xp.full_lists(64, 8), {"wide": 8, "max_p": 64, "max_q": 64, "max_pq": 4096}),
    "full57x9": (lambda: xp.full_lists(57, 9), {"wide": 10, "max_p": 57, "max_q": 57, "max_pq": 3249}),
    "sized768x16": (lambda: xp.sized(768, 16), {"wide": 16, "max_p": 768, "max_q": 52, "max_pq": 12288}),
    "sized128x96": (lambda: xp.sized(128, 96), {"wide": 1, "max_p": 128, "max_q": 96, "max_pq": 12288}),
    "fan1536x8": (lambda: xp.fan(1536, 8), {"wide": 9, "max_p": 1536, "max_q": 192, "max_pq": 12288}),
    "fan1536x8shared": (lambda: xp.fan(1536, 8, shared=True), {"wide": 9, "max_p": 1536, "max_q": 1536, "max_pq": 12288}),
    "fan4096x3": (lambda: xp.fan(4096, 3), {"wide": 4, "max_p": 4096, "max_q": 1366, "max_pq": 12288}),
    "fan6144x2": (lambda: xp.fan(6144, 2), {"wide": 3, "max_p": 6144, "max_q": 3072, "max_pq": 12288}),
    "hub22": (lambda: xp.hub(22), {"wide": 0, "max_p": 23, "max_q": 22, "max_pq": 69}),
    "hub23": (lambda: xp.hub(23), {"wide": 1, "max_p": 24, "max_q": 23, "max_pq": 72}),
    "many_wide1030": (lambda: xp.many_wide(1030), {"wide": 1030, "max_p": 41, "max_q": 40, "max_pq": 123}),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_spai1_accepted(esp, spai, name):
    make, numbers = ACCEPTED[name]
    csc = make()
    assert expected_stats(esp, csc) == numbers
    st, want = tsg.check_all(esp, spai, tsg.from_arrays(esp, csc), arrays=csc)
    assert st == numbers


@pytest.mark.parametrize("name", ["block23", "hub23", "sized128x96"])
def test_spai1_symmetrised(esp, spai, name):
    csc = ACCEPTED[name][0]()
    st, want = tsg.check_all(esp, spai, tsg.from_arrays(esp, csc), True, arrays=csc)
    assert st == ACCEPTED[name][1]
    if name != "block23":                                # (a full block is its own transpose's pattern; the others gain positions)
        assert len(want.M[1]) > len(want.raw[1])


def test_spai1_tridiagonal_past_the_grid(esp, spai):
    """n = 2^20 + 1: the last column is the second turn of workgroup 0 in the size pass and in the numeric pass of the wave tier"""
    csc = xp.tridiagonal(xp.GRID_MAX + 1)
    want = spai.precon(csc, 1, False)
    P = tsg.Spai(esp, tsg.from_arrays(esp, csc))
    try:
        tsg.check_matrix(P, want)
        assert P.stats() == {"wide": 0, "max_p": 5, "max_q": 3, "max_pq": 15}
        v = np.random.default_rng(1).standard_normal(want.n)
        assert tsg.same_bits(P.ldiv(v), want.ldiv(v))
    finally:
        P.close()


# ---- SPAI-1, refused ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,p_text", [(111, "p = 111"), (128, "p = 128"), (129, "p >= 129")])
def test_spai1_refused(esp, spai, m, p_text):
    """tc = 12321 and 16384 (still sorted: the exact p) and 16641 (unsorted: the bound max(maxlen, ceil(tc / q)) = 129); a
    preconditioner updated into that state keeps its earlier M"""
    D = limits(esp)[1]
    bad = xp.dense_block(m)
    text = "%s rows by q = %d unknowns" % (p_text, m)
    with pytest.raises(esp.EspError) as e:
        esp.SPAIPreconditioner(tsg.from_arrays(esp, bad))
    assert e.value.code == ESP_ERR_UNSUPPORTED
    assert "column 0 " in str(e.value) and text in str(e.value) and str(D) in str(e.value)
    good = xp.tridiagonal(m)
    A = tsg.from_arrays(esp, good)
    P = tsg.Spai(esp, A)
    want = spai.precon(good, 1)
    tsg.check_matrix(P, want)
    set_matrix(esp, A, bad)
    with pytest.raises(esp.EspError) as e:
        P.update()
    assert e.value.code == ESP_ERR_UNSUPPORTED and "column 0 " in str(e.value) and text in str(e.value)
    cp, rv, nz = P.matrix()                                                             # the earlier M, untouched
    assert np.array_equal(cp, want.M[0]) and np.array_equal(rv, want.M[1]) and tsg.same_bits(nz, want.M[2])
    st = P.stats()
    assert (st["max_p"], st["max_q"], st["max_pq"], st["wide"]) == want.stats + (0,)
    set_matrix(esp, A, good)                                                            # ... and serves again
    P.update()
    tsg.check_matrix(P, want)
    tsg.check_ldiv(P, want)
    P.close()


# ---- SPAI-1, update! ---------------------------------------------------------------------------------------------------------------
def same_matrix(P, F):
    a, b = P.matrix(), F.matrix()
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tsg.same_bits(a[2], b[2])


@pytest.mark.parametrize("name", ["block110", "sized768x16"])
def test_spai1_values_only_update(esp, spai, name):
    """the numeric pass alone on the kept p, tiers, list and R slots: a fresh create's bits"""
    cp, rv, nz = ACCEPTED[name][0]()
    A = tsg.from_arrays(esp, (cp, rv, nz))
    P = tsg.Spai(esp, A)
    nz2 = nz * (1.0 + 0.25 * np.random.default_rng(3).random(len(nz)))
    set_values(A, nz2)
    P.update()
    want = spai.precon((cp, rv, nz2), 1)
    tsg.check_matrix(P, want)
    assert not tsg.same_bits(want.M[2], spai.precon((cp, rv, nz), 1).M[2])
    F = tsg.Spai(esp, A)
    assert same_matrix(P, F) and P.stats() == F.stats() == ACCEPTED[name][1]
    tsg.check_ldiv(P, want)
    F.close()
    P.close()


def grown_hubs(h0, h1, rng_seed):
    """two blocks: a hub of h0 unknowns in a block of h1 + 1 columns (the columns h0+1..h1 store their diagonal alone) beside
    hub_columns(23); then the first hub grown to the rows 1..h1"""
    first = xp.hub_columns(h0) + [[j] for j in range(h0 + 1, h1 + 1)]
    grown = [list(range(1, h1 + 1))] + first[1:]
    other = xp.hub_columns(23)
    rng = np.random.default_rng(rng_seed)
    return xp.csc_from_columns(xp.block_diagonal([first, other]), rng), xp.csc_from_columns(xp.block_diagonal([grown, other]), rng)


def test_spai1_update_that_raises_wideq(esp, spai):
    """the widest workgroup-tier column grows from q = 23 to q = 40: the R slots grow with it, and the q = 23 column beside it
    computes in a slot sized for 40"""
    before, after = grown_hubs(23, 40, 11)
    assert expected_stats(esp, before) == {"wide": 2, "max_p": 24, "max_q": 23, "max_pq": 72}
    assert expected_stats(esp, after) == {"wide": 2, "max_p": 41, "max_q": 40, "max_pq": 800}      # (p = 41: column 1, which names the hub; p q = 800: the hub, 20 x 40)
    A = tsg.from_arrays(esp, before)
    P = tsg.Spai(esp, A)
    tsg.check_matrix(P, spai.precon(before, 1))
    set_matrix(esp, A, after)
    P.update()
    want = spai.precon(after, 1)
    tsg.check_matrix(P, want)
    F = tsg.Spai(esp, A)
    assert same_matrix(P, F) and P.stats() == F.stats() == expected_stats(esp, after)
    tsg.check_ldiv(P, want)
    F.close()
    P.close()


def test_spai1_update_that_leaves_no_wide_column(esp, spai):
    before = xp.hub(23)
    after = xp.tridiagonal(24)
    A = tsg.from_arrays(esp, before)
    P = tsg.Spai(esp, A)
    assert P.stats()["wide"] == 1
    set_matrix(esp, A, after)
    P.update()
    want = spai.precon(after, 1)
    tsg.check_matrix(P, want)
    F = tsg.Spai(esp, A)
    assert same_matrix(P, F) and P.stats() == F.stats() == {"wide": 0, "max_p": 5, "max_q": 3, "max_pq": 15}
    tsg.check_ldiv(P, want)
    set_matrix(esp, A, before)                           # ... and back: one workgroup-tier column again
    P.update()
    tsg.check_matrix(P, spai.precon(before, 1))
    assert P.stats()["wide"] == 1
    F.close()
    P.close()


# ---- SPAI-0 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [False, True])
def test_spai0_lane_strides(esp, spai, special):
    """columns of 63, 64, 65, 130 and 200 rows; the diagonal in the first stride, in the second, the last entry of the third; no
    diagonal; an empty column; three live waves in the last workgroup; a stored NaN and Inf"""
    csc = xp.spai0_matrix(special)
    with np.errstate(all="ignore"):
        want = spai.precon(csc, 0)
    A = tsg.from_arrays(esp, csc)
    P = esp.SPAIPreconditioner(A, 0)
    assert tsg.same_bits(P.factor(), want.diag)
    tsg.check_ldiv(P, want)
    assert np.isnan(want.diag[200]) and want.diag[180] == 0.0 and np.isnan(want.diag[160]) == special
    nz2 = csc[2] * (1.0 + 0.25 * np.random.default_rng(4).random(len(csc[2])))
    set_values(A, nz2)
    P.update()
    with np.errstate(all="ignore"):
        assert tsg.same_bits(P.factor(), spai.spai0((csc[0], csc[1], nz2)))
    P.close()


# ---- ILUT --------------------------------------------------------------------------------------------------------------------------
ILUT_CASES = {
    "comb200": lambda: xp.comb(200, 12),
    "comb300": lambda: xp.comb(300, 12),
    "comb4200": lambda: xp.comb(4200, 12),
    "pair5merge": lambda: xp.switch_pair(5)[0],
    "pair5lookup": lambda: xp.switch_pair(5)[1],
    "pair31merge": lambda: xp.switch_pair(31)[0],
    "pair31lookup": lambda: xp.switch_pair(31)[1],
}
ILUT_TIERS = {"comb300": (1, 0), "comb4200": (0, 1)}      # (group, stride): the long column is the only one of its tier


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("par", [(0.0, 0, 1), (0.0, 0, 3), (1e-3, 1, 2)])
@pytest.mark.parametrize("name", sorted(ILUT_CASES))
def test_ilut_lookup(esp, ilut, name, par, keep):
    """S, F, the counts, the tiers, the levels and ldiv! the model's, at create and after one values-only update!"""
    (cp, rv, nz), j = ILUT_CASES[name]()
    n = len(cp) - 1
    A = tig.from_arrays(esp, cp, rv, nz)
    with np.errstate(all="ignore"):
        want = ilut.precon((cp, rv, nz), *par, keep_pattern=keep)
    P = esp.ILUTPreconditioner(A, *par, keep_pattern=keep)
    try:
        tig.check_state(esp, P, want)
        tig.check_ldiv(P, want)
        st = P.stats()
        group, stride = ILUT_TIERS.get(name, (0, 0))
        assert (st["wave"], st["group"], st["stride"]) == (n - group - stride, group, stride)
        nz2 = nz * (1.0 + 0.01 * np.random.default_rng(8).random(len(nz)))
        assert A._d.lib.esp_set_nzval(A._d.h, tsg.vp(nz2)) == 0
        P.update()
        want.update((cp, rv, nz2))
        tig.check_state(esp, P, want)
        tig.check_ldiv(P, want, seed=6)
        st = P.stats()
        assert (st["wave"], st["group"], st["stride"]) == (n - group - stride, group, stride)
    finally:
        P.close()
