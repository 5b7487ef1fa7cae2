"""CPU: the cases of tests/consumer_cases.py sit on the edges they are named for -- checked with numpy and the oracle alone, so that
tests/test_consumers_gpu.py cannot pass for the wrong reason, and so that a change of a constant in scan.hpp, radix.hpp or
consumers.hip fails HERE instead of moving a GPU test off its edge."""
import numpy as np
import pytest

import consumer_cases as cc
from refmodel import bits, check_julia_invariants


def _orc_csc(orc, case):
    return orc.CSC(case.m, case.n, case.colptr, case.rowval, case.nzval)


def _valid(case):
    check_julia_invariants(case.m, case.n, case.colptr, case.rowval, case.nzval)


def test_constants_are_the_sources():
    src = cc.source_constants()
    for name, value in src.items():
        assert getattr(cc, name) == value, (name, getattr(cc, name), value)
    assert cc.bits_for(1) == 1 and cc.bits_for(2) == 1 and cc.bits_for(3) == 2 and cc.bits_for(256) == 8 and cc.bits_for(257) == 9


# ------------------------------------------------------------------------------------------------------------ dropzeros!
DROPS = cc.drop_cases()


def test_drop_cases_cover_the_list():
    assert cc.DROP_Z == (1, 2047, 2048, 2049, 3 * 2048 + 5)
    for Z in cc.DROP_Z:
        for which in cc.DROP_SETS:
            case, p = DROPS["drop_Z%d_%s" % (Z, which)]
            _valid(case)
            assert p["Z"] == Z == len(case.nzval)
            want = dict(none=0, all=Z, first=1, last=1, alternate=(Z + 1) // 2)[which]
            assert len(p["drop"]) == want and p["kept"] == Z - want
            if which == "first":
                assert p["drop"].tolist() == [0]
            if which == "last":
                assert p["drop"].tolist() == [Z - 1]
            if which == "alternate":
                assert np.array_equal(p["drop"], np.arange(0, Z, 2))
    # the flags are scanned in chunks of 2048 over Z + 1 slots: Z = 2047 fills one chunk, 2048 spills the sentinel, 2049 an entry
    assert [-(-(Z + 1) // cc.SCAN_CHUNK) for Z in cc.DROP_Z] == [1, 1, 2, 2, 4]


def test_drop_chunk_edges():
    case, p = DROPS["drop_chunk_edges"]
    _valid(case)
    drop = set(p["drop"].tolist())
    assert {2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 0, p["Z"] - 1} == drop
    assert p["chunks"] == [0, 1, 2, 3] and len(p["chunks"]) >= 3
    for run in ((2047, 2049), (4095, 4097), (6143, 6145)):          # a kept entry on either side of every run of drops
        assert run[0] - 1 not in drop and run[1] + 1 not in drop
    assert 1 not in drop and p["Z"] - 2 not in drop
    assert np.all(np.diff(case.colptr)[[0, -1]] > 0)                 # (the first and the last entry belong to stored columns)


def test_drop_random_empty_columns():
    case, p = DROPS["drop_random_empty_columns"]
    _valid(case)
    assert p["empty_before"].tolist() == list(range(1, 6)) + list(range(51, 61)) + list(range(116, 121))
    assert 0.30 < len(p["drop"]) / p["Z"] < 0.40
    assert p["chunks"] == [0, 1, 2, 3]
    assert 77 in p["emptied"].tolist()
    nz_after = np.bincount(cc.coo_of(case)[1][case.nzval != 0.0] - 1, minlength=case.n)
    assert nz_after[75] > 0 and nz_after[76] == 0 and nz_after[77] > 0
    steps = np.diff(p["drop"])
    assert (steps == 1).any() and (steps > 1).any()                   # runs of drops and single drops, in the middle of the arrays


def test_drop_special_values(orc):
    case, p = DROPS["drop_special_values"]
    _valid(case)
    b = bits(case.nzval)
    for v in cc.SPECIAL_VALUES:
        assert (b == bits(np.array([v]))[0]).sum() > 100, v
    O = _orc_csc(orc, case)
    O.dropzeros()
    _, _, nz = O.arrays()
    # both zeros go; NaN, the subnormal, -Inf and 1.5 stay, with their bits
    assert len(nz) == p["kept"] == int(((case.nzval != 0.0) | np.isnan(case.nzval)).sum())
    assert np.array_equal(bits(nz), b[(case.nzval != 0.0)])
    assert np.isnan(nz).sum() > 100 and (nz == 5e-324).sum() > 100 and not (nz == 0.0).any()


def test_drop_rectangular():
    row, pr = DROPS["drop_1xn"]
    col, pc = DROPS["drop_mx1"]
    _valid(row)
    _valid(col)
    assert (row.m, col.n) == (1, 1) and row.n == col.m == 2500
    for case, p in ((row, pr), (col, pc)):
        assert len(p["drop"]) > 400 and p["kept"] > 400 and (bits(case.nzval) == bits(np.array([-0.0]))[0]).sum() > 100
    assert len(pr["emptied"]) == len(pr["drop"]) and pc["emptied"].tolist() == []


@pytest.mark.parametrize("name", ["drop_Z2049_alternate", "drop_chunk_edges", "drop_random_empty_columns", "drop_Z6149_all"])
def test_drop_oracle_and_join_stream(orc, name):
    """the oracle drops what the builder says, and the stream of the flush that follows hits removed, kept and new positions"""
    case, p = DROPS[name]
    O = _orc_csc(orc, case)
    O.dropzeros()
    cp, rv, nz = O.arrays()
    assert len(rv) == p["kept"]
    assert np.all(np.diff(cp)[p["emptied"] - 1] == 0) and np.all(np.diff(case.colptr)[p["emptied"] - 1] > 0)
    kinds, I, J, V = cc.join_stream(case)
    assert set(kinds.tolist()) == {cc.SET, cc.UPDATE, cc.RAWUPDATE} and (V == 0.0).any()
    r, c = cc.coo_of(case)
    stored = dict(zip(zip(r.tolist(), c.tolist()), (case.nzval == 0.0).tolist()))
    hit = [stored.get(ij) for ij in zip(I.tolist(), J.tolist())]
    assert (hit.count(False) >= 50 or p["kept"] == 0) and hit.count(None) >= 50
    assert hit.count(True) >= 50 or len(p["drop"]) == 0


# -------------------------------------------------------------------------------------------------------------- getindex
def test_getindex_case(orc):
    case, p = cc.getindex_case()
    _valid(case)
    assert set(p["types"]) == set(cc.GETINDEX_COLUMN_TYPES)
    assert p["types"][0] == p["types"][-1] == "empty" and "empty" in p["types"][1:-1]
    O = _orc_csc(orc, case)
    look = cc.getindex_lookups(case)
    found = {ij: O.findindex(*ij) for ij in look}
    for j, t in enumerate(p["types"], 1):
        mine = [i for (i, jj) in look if jj == j]
        assert 1 in mine and case.m in mine
        rows = case.rowval[case.colptr[j - 1] - 1: case.colptr[j] - 1]
        assert len(rows) == dict(empty=0, one=1, two=2, three=3, sixty_four=64, dense=case.m)[t]
        if len(rows):
            assert rows[0] in mine and rows[-1] in mine
        if 0 < len(rows) <= 3:
            assert all(r in mine for r in rows)
        hits = [i for i in mine if found[(i, j)] > 0]
        assert len(hits) == len(set(mine) & set(rows.tolist()))
        if 0 < len(rows) < case.m:
            assert any(found[(i, j)] == 0 for i in mine), "a row just beside a stored one is absent"
    k0, k1, k2 = O.findindex(*p["zero_at"]), O.findindex(*p["negzero_at"]), O.findindex(*p["dense_zero_at"])
    assert k0 > 0 and k1 > 0 and k2 > 0
    assert bits(case.nzval[[k0 - 1, k1 - 1, k2 - 1]]).tolist() == bits(np.array([0.0, -0.0, 0.0])).tolist()
    assert p["zero_at"] in look and p["negzero_at"] in look
    # absent first / last rows exist too
    assert any(found[(1, j)] == 0 for j in range(1, case.n + 1)) and any(found[(case.m, j)] == 0 for j in range(1, case.n + 1))


# ------------------------------------------------------------------------------------------------ getindex of the pending buffer
def _oracle_pending(orc, kinds, I, J, V):
    O = orc.ExtendableSparseMatrix(cc.PENDING_M, cc.PENDING_N)
    O.apply(kinds, I, J, V)
    return O


def test_pending_k_list():
    cap = cc.PENDING_MATCH_CAP
    assert cc.PENDING_K == (1, 255, 256, 257, cap - 1, cap) and cc.PENDING_FOLD_THREADS == 256
    assert cc.PENDING_NOISE // 256 > 500                         # many workgroups of pending_matches_k


@pytest.mark.parametrize("k", cc.PENDING_K + (cc.PENDING_MATCH_CAP + 1, 0))
def test_pending_stream(orc, k):
    (kinds, I, J, V), p = cc.pending_stream(k)
    i, j = p["target"]
    at = np.flatnonzero((I == i) & (J == j))
    assert len(at) == k and np.array_equal(at, p["at"])          # exactly k matches of the target
    assert p["groups"] > 500
    if k > 1:
        assert len(set((at // 256).tolist())) > min(k, 700) // 2     # ... from many workgroups
    tk, tv = (cc.target_calls(k) if k else (np.empty(0, np.uint8), np.empty(0)))
    assert np.array_equal(kinds[at], tk) and np.array_equal(bits(V[at]), bits(tv))
    assert set(bits(V).tolist()) == set(bits(np.array(cc.PENDING_VALUES)).tolist())
    if k >= 16:
        assert set(tk.tolist()) == {cc.SET, cc.UPDATE, cc.RAWUPDATE}
        assert set(bits(tv).tolist()) == set(bits(np.array(cc.PENDING_VALUES)).tolist())
    # the oracle's getindex on the pending calls is the fold of the target's calls in call order
    O = _oracle_pending(orc, kinds, I, J, V)
    assert O.pending() > 0
    present, want = cc.fold(tk, tv)
    assert bits(np.array([O[i, j]]))[0] == bits(np.array([want]))[0]
    assert present == (k > 0)
    if k == 1:
        assert bits(np.array([want]))[0] == 0                    # +0.0 from RAWUPDATE -0.0


@pytest.mark.parametrize("k", [255, 256, 257, 2047, 2048])
def test_pending_order_matters(orc, k):
    """what a fold in another order gives: the swap of the head's -1e300 and SET, the reversed order, shuffles, a lost and a doubled call, and the order
    a rank sort that stops after its first stride would leave -- each differs from the call order's result (also on the oracle)"""
    tk, tv = cc.target_calls(k)
    base = cc.fold(tk, tv)

    def variant(order):
        order = np.asarray(order)
        return cc.fold(tk[order], tv[order])

    idx = np.arange(k)
    o = idx.copy()
    o[4], o[5] = o[5], o[4]                                      # UPDATE -1e300 and SET 2^-60
    assert variant(o) != base
    assert variant(idx[::-1]) != base
    rng = np.random.default_rng(k)
    shuffled = [rng.permutation(k) for _ in range(5)]
    for o in shuffled:
        assert variant(o) != base
    ones = np.flatnonzero(tv == 1.0)
    for q in (ones[1], ones[len(ones) // 2], ones[-1]):
        assert variant(np.delete(idx, q)) != base                # a lost 1.0
        assert variant(np.insert(idx, q, q)) != base             # a doubled 1.0
    # matches that arrive in the order `arrive`; a sort that ranks the first 256 arrivals only leaves the others where they are
    arrive = shuffled[0]
    if k >= 2047:                                                # (k = 257 leaves ONE call out of place: it may be a 2^-60 that no sum keeps)
        first = np.sort(arrive[:256])
        assert variant(np.concatenate([first, arrive[256:]])) != base
    # the oracle folds a shuffled call order to something else as well
    i, j = cc.PENDING_TARGET
    O = orc.ExtendableSparseMatrix(cc.PENDING_M, cc.PENDING_N)
    O.apply(tk[arrive], np.full(k, i), np.full(k, j), tv[arrive])
    assert bits(np.array([O[i, j]]))[0] != bits(np.array([base[1]]))[0]


# ----------------------------------------------------------------------------------------- mul! and the row-wise index
MULS = cc.mul_cases()


def test_mul_row_bits():
    assert cc.MUL_M == (1, 2, 255, 256, 257, 65536, 65537, 2 ** 24 + 1)
    want = {1: [1], 2: [1], 255: [8], 256: [8], 257: [8, 1], 65536: [8, 8], 65537: [8, 8, 1], 2 ** 24 + 1: [8, 8, 8, 1]}
    for m in cc.MUL_M:
        case, p = MULS["mul_m%d" % m]
        _valid(case)
        assert case.m == m and p["passes"] == want[m] and p["row_bits"] == sum(want[m])
        rows = set(case.rowval.tolist())
        assert 1 in rows and m in rows                           # the lowest and the highest row: every bit of the key decides
        if m > 1:
            top = 1 << (p["row_bits"] - 1)
            assert any((r - 1) & top for r in rows) and any(not ((r - 1) & top) for r in rows)
        if m < 2 ** 20:
            assert 4990 <= len(case.nzval) <= 5020
        else:
            assert case.n == 7 and 250 <= len(case.nzval) <= 400
        if m >= 255:
            assert np.diff(case.colptr).max() >= 2 and len(rows) > 100


def test_mul_counts_and_shapes():
    assert cc.MUL_Z == (0, 1, cc.SORT_TILE - 1, cc.SORT_TILE, cc.SORT_TILE + 1)
    for Z in cc.MUL_Z:
        case, p = MULS["mul_Z%d" % Z]
        _valid(case)
        assert len(case.nzval) == Z and p["tiles"] == {0: 0, 1: 1, 4095: 1, 4096: 1, 4097: 2}[Z]
    one, p = MULS["mul_one_row"]
    _valid(one)
    assert (one.m, one.n) == (300, 9000) and set(one.rowval.tolist()) == {p["row"]} and len(one.rowval) == 9000 > 2 * cc.SORT_TILE
    dense, p = MULS["mul_dense_column"]
    _valid(dense)
    assert np.diff(dense.colptr)[p["column"] - 1] == dense.m
    edge, p = MULS["mul_empty_edge_rows"]
    _valid(edge)
    rows = set(edge.rowval.tolist())
    assert not rows & set(p["empty"]) and {2, 699} <= rows and p["empty"] == (1, 350, 700)
    assert (MULS["mul_n0"][0].m, MULS["mul_n0"][0].n, MULS["mul_m0"][0].m, MULS["mul_m0"][0].n) == (5, 0, 0, 5)


def test_mul_nonfinite(orc):
    (case, x), p = cc.mul_nonfinite()
    _valid(case)
    assert np.isposinf(x[6]) and np.isneginf(x[10]) and np.isnan(x[12]) and np.isnan(x[7 * 13 - 1])
    assert np.array_equal(np.flatnonzero(~np.isfinite(x)) + 1, p["special"])
    _, cols = cc.coo_of(case)
    at = np.isin(cols, p["special"])
    zero_there = at & (case.nzval == 0.0)
    assert zero_there.sum() > 300 and (at & (case.nzval != 0.0)).sum() > 100
    assert (bits(case.nzval[zero_there]) == 0).any() and (bits(case.nzval[zero_there]) != 0).any()     # 0.0 and -0.0
    r = _orc_csc(orc, case).mul(x)
    # 0 * Inf = NaN: the rows that hold nothing but stored zeros there are NaN; skipping stored zeros would make them 0.0
    assert np.isnan(r[p["zero_rows"] - 1]).all()
    skipped = cc.csc_from_coo("skipped", case.m, case.n, case.rowval[case.nzval != 0.0], cols[case.nzval != 0.0], case.nzval[case.nzval != 0.0])
    r2 = _orc_csc(orc, skipped).mul(x)
    assert (r2[p["zero_rows"] - 1] == 0.0).all() and (np.isnan(r) != np.isnan(r2)).sum() >= 10
    assert np.isfinite(r).any() and np.isinf(r).any()


def test_mul_negzero(orc):
    (case, x), p = cc.mul_negzero()
    _valid(case)
    rows, cols = cc.coo_of(case)
    prod = case.nzval * x[cols - 1]
    low = np.isin(rows, p["rows"])
    assert low.sum() > 300 and (bits(prod[low]) == bits(np.array([-0.0]))[0]).all()
    r = _orc_csc(orc, case).mul(x)
    stored = np.isin(p["rows"], rows)
    assert stored.all() and (bits(r[p["rows"] - 1]) == 0).all()       # +0.0: acc starts at +0.0
    assert (r[32:] != 0.0).all()


# ------------------------------------------------------------------------------------------- every editor x every reader
def test_editor_cases(orc):
    assert cc.EDITOR_N > cc.LAZY_COLPTR_N and set(cc.EDITORS) == set(cc.EDITOR_EFFECT)
    base, p = cc.editor_base(zeros=True)
    plain, _ = cc.editor_base(zeros=False)
    _valid(base)
    _valid(plain)
    assert (base.nzval == 0.0).sum() > 2000 and not (plain.nzval == 0.0).any()
    assert np.array_equal(base.colptr, plain.colptr) and np.array_equal(base.rowval, plain.rowval)
    stored, val = cc.diagonal_of(base)
    assert (~stored).sum() == cc.EDITOR_N // 10 and p["marked"] > 100
    O = _orc_csc(orc, base)
    marker = O.mark_dirichlet()
    assert 100 < marker.sum() < cc.EDITOR_N // 10 and np.array_equal(marker, stored & (val >= cc.PENALTY))
    inv = O.jacobi()
    assert np.isinf(inv).sum() >= (~stored).sum() and np.isfinite(inv).sum() > 3500
    other, _ = cc.editor_other()
    _valid(other)
    assert not np.array_equal(other.colptr, base.colptr)
    _, I, J, _ = cc.editor_hits(base)
    assert cc.stored_fraction(base, I, J) == 1.0
    _, I, J, _ = cc.editor_adds(base)
    assert cc.stored_fraction(base, I, J) < 0.01
    _, I, J, _ = cc.window_stream()
    assert J.min() >= cc.WINDOW[0] and J.max() <= cc.WINDOW[1] < cc.EDITOR_N and cc.WINDOW[0] > 1
    for n in (cc.LAZY_COLPTR_N, cc.LAZY_COLPTR_N + 1):
        d, _ = cc.diagonal_case(n)
        _valid(d)
        assert np.array_equal(d.colptr, np.arange(1, n + 2))       # nothing like the all-ones colptr of the empty matrix


# -------------------------------------------------------------------------------------- Dirichlet helpers, diagonal set-up
@pytest.mark.parametrize("n", cc.DIRICHLET_N)
def test_dirichlet_case(orc, n):
    assert cc.DIRICHLET_N == (1, 255, 256, 257)
    case, p = cc.dirichlet_case(n)
    _valid(case)
    stored, val = cc.diagonal_of(case)
    O = _orc_csc(orc, case)
    marker = O.mark_dirichlet()
    assert np.array_equal(np.flatnonzero(marker) + 1, p["marked"])
    if n == 1:
        assert val[0] == cc.PENALTY and marker.tolist() == [True]
        return
    assert np.array_equal(np.flatnonzero(~stored) + 1, p["missing"]) and len(p["missing"]) >= 30 and p["missing"][0] == 9
    assert (val[stored] == cc.PENALTY).sum() >= 30 and (val[stored] > cc.PENALTY).sum() >= 30       # == penalty: the >= of the reference
    nan = stored & np.isnan(val)
    assert nan.sum() >= 15 and not marker[nan].any()
    zero = stored & (val == 0.0)
    assert (bits(val[zero]) == 0).sum() >= 15 and (bits(val[zero]) != 0).sum() >= 15
    rows, cols = cc.coo_of(case)
    off = rows != cols
    big = off & (case.nzval >= cc.PENALTY)
    assert big.sum() >= 10 and not marker[np.setdiff1d(cols[big], p["marked"]) - 1].any()       # a large off-diagonal entry marks nothing
    assert (off & (case.nzval == 0.0)).sum() >= 100
    for k in p["marked"]:                                             # rows and columns of a marked node both hold entries
        assert (off & (cols == k)).any() and (off & (rows == k)).any()
    inv = O.jacobi()
    assert np.isposinf(inv[~stored]).all() and np.isnan(inv[nan]).all()
    assert np.isposinf(inv[zero & (bits(val) == 0)]).all() and np.isneginf(inv[zero & (bits(val) != 0)]).all()
    with pytest.raises(ValueError, match="column 9 "):
        O.ilu0()
    # stored zeros stay structural after elimination
    before = O.arrays()
    O.eliminate_dirichlet(marker)
    after = O.arrays()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (after[2] == 0.0).sum() > (before[2] == 0.0).sum()
    full, pf = cc.dirichlet_case(n, full_diagonal=True)
    _valid(full)
    assert len(pf["missing"]) == 0 and cc.diagonal_of(full)[0].all()
    xd, idg = _orc_csc(orc, full).ilu0()
    assert np.isfinite(xd).all() and (idg > 0).all()
