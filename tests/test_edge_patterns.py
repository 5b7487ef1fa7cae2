"""CPU: the crafted patterns of tests/edge_patterns.py are what they claim to be -- the prescribed schedule of every layered
pattern has exactly the prescribed level widths (by iluam_modellib's NumPy restatement of the schedules), launch_list gives the
hand-written launch counts, the capacity matrix holds its table of per-block entry counts (counted with SciPy), and the C
models' factorizations and ldiv! on every pattern are finite.  The second half does the same for tests/algebra_patterns.py: the
column lengths, the position of every tile border relative to the column starts, the merged positions of the A+-B pairs (by a plain
Python merge), the tiles and columns of the model's result that are empty, and finite, non-trivial model results."""
import numpy as np
import pytest
import scipy.sparse as sp

import edge_patterns as ep
from iluam_modellib import Model, level_schedules
from precon_modellib import Model as PreconModel


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("edge_iluam_model"))


@pytest.fixture(scope="module")
def precon_model(tmp_path_factory):
    return PreconModel(tmp_path_factory.mktemp("edge_precon_model"))


@pytest.mark.parametrize("form", ep.FORMS)
@pytest.mark.parametrize("name", sorted(ep.WIDTHS))
def test_layered_widths_and_finite_model(model, name, form):
    widths = ep.WIDTHS[name]
    I, J, V, n = ep.layered(widths, form, seed=3)
    assert n == sum(widths) and len(I) == len(J) == len(V)
    assert len(np.unique((I - 1) * n + (J - 1))) == len(I)                    # unique triplets
    assert I.min() >= 1 and I.max() <= n and J.min() >= 1 and J.max() <= n
    off = V[I != J]
    assert np.all(np.abs(off) < 1.0)
    arrays = ep.csc_arrays(n, I, J, V)
    sched = level_schedules(arrays[0], arrays[1])
    for k in ep.PRESCRIBED[form]:
        assert ep.widths_of(sched[k]) == widths
    # every diagonal entry is 1 + max(row abs sum, column abs sum)
    S = sp.csc_matrix((arrays[2], arrays[1] - 1, arrays[0] - 1), shape=(n, n))
    A = abs(S)
    d = S.diagonal()
    rows = np.asarray(A.sum(axis=1)).ravel() - d
    cols = np.asarray(A.sum(axis=0)).ravel() - d
    np.testing.assert_allclose(d, 1.0 + np.maximum(rows, cols), rtol=1e-14, atol=0)
    f, diag = model.factor(arrays)
    assert np.isfinite(f).all()
    u = model.ldiv(arrays, f, diag, np.random.default_rng(1).standard_normal(n))
    assert np.isfinite(u).all()


def test_mixed_is_what_the_launch_tests_need():
    widths = ep.WIDTHS["mixed"]
    assert sum(widths) == 1801
    assert ep.launch_list(widths) == (3, 6)       # [128 128] [1] [256] 257 [1 1] 512 [3] 513 [1]: thin in brackets
    I, J, V, n = ep.layered(widths, "symmetric", seed=3)
    S = sp.csr_matrix((np.ones(len(I)), (I - 1, J - 1)), shape=(n, n))
    # the single node in front of the level of 512: its dependents and the diagonal
    assert np.diff(S.indptr).max() >= 513 and np.diff(S.tocsc().indptr).max() >= 513


def test_launch_list_by_hand():
    assert ep.launch_list(ep.WIDTHS["fold_exact"]) == (0, 2)     # 255 + 1 = 256 fold, then 1
    assert ep.launch_list(ep.WIDTHS["fold_exact2"]) == (0, 2)    # 1 + 255 = 256 fold, then 1
    assert ep.launch_list(ep.WIDTHS["fold_over"]) == (0, 2)      # 255 + 2 = 257 does not fold: [255] [2 1]
    assert ep.launch_list(ep.WIDTHS["w256"]) == (0, 1)
    assert ep.launch_list(ep.WIDTHS["w257"]) == (1, 0)
    assert ep.launch_list(ep.WIDTHS["chain300"]) == (0, 2)       # 256 levels of one node, then 44
    assert ep.launch_list(ep.WIDTHS["pairs129"]) == (0, 2)       # 128 levels of two nodes, then one
    assert ep.launch_list([]) == (0, 0)
    assert ep.launch_list([257, 256, 1, 257]) == (2, 2)          # 256 + 1 does not fold


def test_launch_list_on_the_recorded_colourings():
    """NOTES/coloring.md: the colour members of fdrand 64^3 (19 levels -> 15 launches per schedule) and of 128^3 (20 -> 17)"""
    m64 = [38127, 34734, 30645, 29891, 27663, 26351, 23109, 19130, 14054, 9236, 5145, 2455, 1050, 378, 121, 41, 10, 3, 1]
    assert sum(m64) == 64 ** 3 and len(m64) == 19
    assert sum(ep.launch_list(m64)) == 15 and ep.launch_list(m64) == (14, 1)
    m128 = [301501, 274492, 243382, 236342, 220622, 208443, 185245, 154590, 115350, 76020, 43754, 22023, 9604, 3803, 1372, 437, 117,
            42, 11, 2]
    assert sum(m128) == 128 ** 3 and len(m128) == 20
    assert sum(ep.launch_list(m128)) == 17


@pytest.fixture(scope="module")
def capacity():
    I, J, V, n = ep.capacity(seed=7)
    return I, J, V, n, ep.csc_arrays(n, I, J, V)


def test_capacity_table(capacity):
    I, J, V, n, arrays = capacity
    assert n == 2341 == ep.CAPACITY_N
    assert len(np.unique((I - 1) * n + (J - 1))) == len(I)
    S = sp.csr_matrix((V, (I - 1, J - 1)), shape=(n, n))
    assert S.nnz == len(I)
    want_total = [4352, 4352, 4352, 2047, 2048, 2049, 2356, 256, 1256, 2220]
    for blk, (nl, nu) in enumerate(ep.CAPACITY_BLOCKS):
        r0, r1 = blk * 256, min((blk + 1) * 256, n)
        B = S[r0:r1].tocoo()
        rows = B.row + r0
        low, up, dia = int((B.col < rows).sum()), int((B.col > rows).sum()), int((B.col == rows).sum())
        assert (low, up, dia) == (nl, nu, r1 - r0), blk
        assert low + up + dia == want_total[blk] == S.indptr[r1] - S.indptr[r0]
    per_row = np.diff(S.indptr)
    assert per_row[6 * 256] == 2101 and np.all(per_row[6 * 256 + 1:7 * 256] == 1)     # a single row above the capacity
    assert np.all(per_row[7 * 256:8 * 256] == 1)                                      # empty parts
    assert np.all(per_row[9 * 256:] == 60) and n - 9 * 256 == 37                      # the ragged last block: 59 lower + diagonal
    # the table's edges against the capacity itself
    assert [t - ep.CAP for t in want_total[3:6]] == [-1, 0, 1]
    assert [ep.CAPACITY_BLOCKS[b][0] - ep.CAP for b in range(3)] == [-1, 0, 1]
    assert [ep.CAPACITY_BLOCKS[b][1] - ep.CAP for b in range(3)] == [1, 0, -1]
    # spread as evenly as the room allows: inside a block the counts of rows with room differ by at most one
    T = S.tocoo()
    lrow = np.bincount(T.row[T.col < T.row], minlength=n)
    for blk in (1, 2, 3, 4, 5, 8, 9):
        c = lrow[blk * 256:min((blk + 1) * 256, n)]
        assert c.max() - c.min() <= 1
    c0 = lrow[:256]                                                                    # block 0: row r has room for r only
    full = c0 == np.arange(256)
    assert c0[full].max() <= c0[~full].max() and c0[~full].max() - c0[~full].min() <= 1
    # the diagonal is 1 + row abs sum
    A = abs(S)
    d = S.diagonal()
    np.testing.assert_allclose(d, 1.0 + (np.asarray(A.sum(axis=1)).ravel() - d), rtol=1e-14, atol=0)


def test_capacity_models_are_finite(orc, model, precon_model, capacity):
    I, J, V, n, arrays = capacity
    cp, rv, nz = arrays
    v = np.random.default_rng(2).standard_normal(n)
    C = orc.CSC(n, n, cp, rv, nz)
    xd, idg = C.ilu0()
    assert np.isfinite(np.asarray(xd)).all() and np.isfinite(np.asarray(C.jacobi())).all()
    assert np.isfinite(precon_model.ilu0_ldiv(arrays, xd, idg, v)).all()
    assert np.isfinite(precon_model.mul(arrays, v)).all()
    f, diag = model.factor(arrays)
    assert np.isfinite(f).all() and np.isfinite(model.ldiv(arrays, f, diag, v)).all()


def test_tridiagonal_triplets():
    I, J, V = ep.tridiagonal_triplets(5)
    S = sp.csr_matrix((V, (I - 1, J - 1)), shape=(5, 5)).toarray()
    assert np.array_equal(S, 4.0 * np.eye(5) - 1.5 * np.eye(5, k=-1) - 0.5 * np.eye(5, k=1))
    assert all(len(a) == 0 for a in ep.tridiagonal_triplets(0))
    assert [len(a) for a in ep.tridiagonal_triplets(1)] == [1, 1, 1]


# ---- tests/algebra_patterns.py: the algebra and set-up side ---------------------------------------------------------------------
import math  # noqa: E402

import algebra_patterns as ap  # noqa: E402
import amg_modellib as am  # noqa: E402
import iluk_modellib  # noqa: E402
import linalg_modellib  # noqa: E402
import matops_modellib  # noqa: E402
from block_precon_modellib import block_matrix  # noqa: E402
from refmodel import bits  # noqa: E402


@pytest.fixture(scope="module")
def linalg(tmp_path_factory):
    return linalg_modellib.Model(tmp_path_factory.mktemp("edge_linalg_model"))


@pytest.fixture(scope="module")
def matops(tmp_path_factory):
    return matops_modellib.Model(tmp_path_factory.mktemp("edge_matops_model"))


def check_csc(csc, m):
    cp, rv, nz = csc
    assert cp[0] == 1 and cp[-1] == len(rv) + 1 == len(nz) + 1 and np.all(np.diff(cp) >= 0)
    assert len(rv) == 0 or (rv.min() >= 1 and rv.max() <= m)
    for j in np.flatnonzero(np.diff(cp) > 1):
        assert np.all(np.diff(rv[cp[j] - 1:cp[j + 1] - 1]) > 0)         # rows ascending and distinct


def has_specials(nz):
    b = bits(np.asarray(nz))
    return all(np.any(b == bits(np.array([s]))[0]) for s in (0.0, ap.NEG_ZERO, ap.NAN_PAYLOAD))


def test_prescribed_lengths(linalg):
    subs = ap.sort_sublists()
    assert sorted(subs) == ap.SORT_MAXIMA == [8, 9, 16, 17, 32, 33, 4096, 4097]
    assert subs[4096] == ap.SORT_LENGTHS and subs[4097] == ap.SORT_LENGTHS + [4097] and subs[8] == [0, 1, 2, 7, 8]
    assert (ap.COLSORT_LANE, ap.COLSORT_BLOCK) == (32, 4096)
    for mx, lengths in subs.items():
        assert max(lengths) == mx
        csc = ap.prescribed_lengths(lengths, seed=mx)
        check_csc(csc, ap.SORT_ROWS)
        assert list(np.diff(csc[0])) == lengths
        assert sum(l > ap.COLSORT_LANE for l in lengths) == {32: 0, 33: 1}.get(mx, sum(l > 32 for l in lengths))
        assert has_specials(csc[2])
        j = int(np.argmax(lengths))
        col = csc[1][csc[0][j] - 1:csc[0][j + 1] - 1]
        assert col.max() - col.min() > ap.SORT_ROWS // 2                     # spread over the row range
        # the operand of the device transpose: its rows are the prescribed columns
        T = ap.transpose_csc(ap.SORT_ROWS, csc)
        check_csc(T, len(lengths))
        back = linalg.transpose(len(lengths), T)
        assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
                   for a, b in zip(back, csc))
    # the workgroup sort's padded size S: 64 at 33, 4096 at 4096
    for L, S in ((33, 64), (4096, 4096)):
        s = 2
        while s < L:
            s <<= 1
        assert s == S


def test_prescribed_square_and_partitions():
    for mx, lengths in ap.sort_sublists().items():
        lengths = [l for l in lengths if l >= 1]
        csc, n, where = ap.prescribed_square(lengths, seed=mx)
        check_csc(csc, n)
        lens = np.diff(csc[0])
        assert [int(lens[c]) for c in where] == lengths and max(lengths) == mx      # the diagonal added, the lengths kept
        assert np.all(np.delete(lens, where) == 1) and n >= mx + 3
        cols = np.repeat(np.arange(n), lens)
        assert np.count_nonzero(csc[1] - 1 == cols) == n                             # a full diagonal
        assert np.isfinite(csc[2]).all() and np.any(bits(csc[2]) == bits(np.array([-0.0]))[0])
        parts = ap.worst_case_partitions(n)
        assert sorted(parts) == ["reversed", "shuffled", "zigzag"]
        for name, p in parts.items():
            assert np.array_equal(np.sort(np.concatenate(p)), np.arange(n))
        # what reaches the sorts: the new rows of a column in stored order
        new = np.empty(n, np.int64)
        new[parts["reversed"][0]] = np.arange(n)
        c = where[-1]
        assert np.all(np.diff(new[csc[1][csc[0][c] - 1:csc[0][c + 1] - 1] - 1]) < 0)   # strictly descending
        new[np.concatenate(parts["zigzag"])] = np.arange(n)
        d = np.diff(new[csc[1][csc[0][c] - 1:csc[0][c + 1] - 1] - 1])
        assert mx < 8 or (np.any(d < 0) and np.any(d > 0))
    csc, n, where = ap.prescribed_square([1, 2, 7, 8], seed=8)
    wcp = block_matrix(csc, ap.worst_case_partitions(n)["reversed"], True)[0]          # one partition keeps every entry
    assert sorted(np.diff(wcp))[-3:] == [2, 7, 8] and wcp[-1] - 1 == len(csc[1])


def test_compaction_edges():
    csc, n, parts = ap.compaction_edges()
    check_csc(csc, n)
    assert ap.BK_LONG == 32 and n == 200
    lens = np.diff(csc[0])
    wcp = block_matrix(csc, parts, False)[0]
    for t, (stored, kept) in enumerate(ap.BK_CASES):
        assert lens[t] == stored and wcp[t + 1] - wcp[t] == kept
        rows = csc[1][csc[0][t] - 1:csc[0][t + 1] - 1] - 1
        mine = rows % 2 == t % 2
        if 0 < kept < stored:
            assert np.any(mine[1:] != mine[:-1])                    # dropped and kept entries interleave
            assert np.count_nonzero(mine[1:] != mine[:-1]) >= 2 * min(kept, stored - kept) - 1
    assert {s for s, _ in ap.BK_CASES} == {32, 33} and {k for s, k in ap.BK_CASES if s == 33} == {0, 1, 16, 31, 32, 33}
    t = ap.BK_CASES.index((33, 33))
    assert has_specials(csc[2][csc[0][t] - 1:csc[0][t + 1] - 1])


def test_bordered():
    cp, rv, nz = ap.bordered()
    check_csc((cp, rv, nz), ap.BORDERED_ROWS)
    lens = list(np.diff(cp))
    nnz = len(rv)
    assert len(lens) == 40 and nnz == 5 * ap.TILE + 1 and ap.TILE == 2048
    assert lens[:2] == [0, 0] and lens[-4:] == [0, 0, 0, 0] and lens[-5] == 1
    assert lens[2] == 2048 and cp[2] - 1 == 0 and cp[3] - 1 == 2048              # one column is exactly the first tile
    assert 4095 in lens
    start, end = cp[:-1] - 1, cp[1:] - 1
    where = {}
    for b in range(ap.TILE, nnz, ap.TILE):
        j = ap.column_of(cp, b)
        where[b] = (j, b - start[j], end[j] - b)                                  # (column, entries before b, entries from b on)
    assert where[2048] == (6, 0, 1000) and lens[3:6] == [0, 0, 0]                 # a column start behind three empty columns
    assert where[4096][0] == 8 and where[4096][1] > 0 and where[4096][2] > 1      # the middle of the column of 4095
    assert where[6144][0] == 8 and where[6144][1] > 0 and where[6144][2] > 1
    assert where[8192][2] == 1 and where[8192][1] == lens[where[8192][0]] - 1     # one entry before a column end
    assert where[10240] == (35, 0, 1) and 10240 == nnz - 1                        # the last tile holds a single entry
    assert has_specials(nz)


def test_symmetric_bordered(linalg):
    csc = ap.symmetric_bordered()
    cp, rv, nz = csc
    n = ap.SYM_N
    check_csc(csc, n)
    assert len(cp) == n + 1 and len(rv) == 3 * ap.TILE + 1
    positions = ap.SYM_POSITIONS + [len(rv) - 1]
    assert positions == [0, 2047, 2048, 4095, 4096, 6144]
    assert linalg.issymmetric(n, csc)
    zeros = np.flatnonzero(nz == 0.0)
    assert len(zeros) == 5 and all(ap.mirror_position(csc, int(p)) < 0 for p in zeros)     # stored zeros without a mirror
    for p in range(len(rv)):
        q = ap.mirror_position(csc, p)
        if p not in zeros:
            assert q >= 0 and bits(nz[q:q + 1])[0] == bits(nz[p:p + 1])[0]
    for p in positions:
        assert rv[p] - 1 != ap.column_of(cp, p) and nz[p] != 0.0
        P = ap.perturbed(csc, p)
        assert np.count_nonzero(bits(P[2]) != bits(nz)) == 1 and bits(P[2])[p] != bits(nz)[p]
        assert not linalg.issymmetric(n, P)
        Z = ap.zero_pair(csc, p)
        assert np.count_nonzero(bits(Z[2]) != bits(nz)) == 2 and linalg.issymmetric(n, Z)
        q = ap.mirror_position(csc, p)
        assert {bits(Z[2][p:p + 1])[0], bits(Z[2][q:q + 1])[0]} == {0, 1 << 63}


def test_merge_cases(matops):
    cases = ap.merge_cases()
    assert ap.MM_TILE == 1024
    for name, c in cases.items():
        A, B, m = c["A"], c["B"], c["m"]
        check_csc(A, m)
        check_csc(B, m)
        assert len(A[0]) == len(B[0]) and len(A[1]) + len(B[1]) == c["total"], name
        st = ap.merged_stream(A, B)
        assert len(st) == c["total"]
        ntiles = (c["total"] + 1023) // 1024
        for sub, op in ((False, "+"), (True, "-")):
            kept = ap.kept_per_tile(A, B, sub)
            got = matops.add(A, B, matops_modellib.OP_SUB if sub else matops_modellib.OP_ADD)
            assert sum(kept) == len(got[1]) > 0 and len(kept) == ntiles, (name, op)
            assert np.isfinite(got[2]).all()
            empty = [t for t, k in enumerate(kept) if k == 0]
            assert empty == c.get("empty_tiles", {}).get(op, []), (name, op)
            gone = [int(j) for j in np.flatnonzero(np.diff(got[0]) == 0)
                    if A[0][j + 1] > A[0][j] or B[0][j + 1] > B[0][j]]                     # stored in an operand, empty in the result
            assert gone == c.get("empty_columns", {}).get(op, []), (name, op)
            if "cancels" in c:                                                             # exactly the split pair of this operation
                row = c["cancels"][op]
                assert len(got[1]) == 1100 - 1 and row not in got[1] and c["cancels"]["-" if op == "+" else "+"] in got[1]
        if "split_pairs" in c:
            for (pa, pb), row in zip(c["split_pairs"], c["split_rows"]):
                assert st[pa][:3] == (0, row, 0) and st[pb][:3] == (0, row, 1)
                assert pa % 1024 == 1023 and pb % 1024 == 0                                # a tile border between the halves
        if "only" in c:
            src, tiles = c["only"]
            for t in range(ntiles):
                srcs = {e[2] for e in st[t * 1024:(t + 1) * 1024]}
                assert (srcs == {src}) == (t in tiles), (name, t)
        if "border" in c:
            d, before, after = c["border"]
            assert d % 1024 == 0 and st[d - 1][0] == before and st[d][0] == after
            la, lb = np.diff(A[0]), np.diff(B[0])
            assert [int(j) for j in np.flatnonzero(la == 0)] == c["empty_a"]
            assert [int(j) for j in np.flatnonzero(lb == 0)] == c["empty_b"]
            only_a = [j for j in range(8) if la[j] == 0 and lb[j] > 0]
            only_b = [j for j in range(8) if lb[j] == 0 and la[j] > 0]
            both = [j for j in range(8) if la[j] == 0 and lb[j] == 0]
            for group in (only_a, only_b, both):                                           # on either side of the border
                assert any(j <= before or before < j < after and j == 3 for j in group), group
                assert any(j >= after or j == 4 for j in group), group
            assert both == [3, 4] and only_a == [1, 5] and only_b == [2, 6]
    assert [cases["total%d" % t]["total"] for t in (1024, 1025, 2048, 2049)] == [1024, 1025, 2048, 2049]
    # a cancelled whole tile lies between tiles that keep entries
    assert ap.kept_per_tile(cases["tile_cancels_add"]["A"], cases["tile_cancels_add"]["B"], False) == [512, 0, 512]
    assert ap.kept_per_tile(cases["tile_cancels_sub"]["A"], cases["tile_cancels_sub"]["B"], True) == [512, 0, 512]
    assert cases["columns_cancel_add"]["empty_columns"]["+"] == [0, 2, 4, 5, 6, 8, 11]      # first, last, a run of three


def test_wave_columns(linalg):
    csc, lengths = ap.wave_columns()
    check_csc(csc, ap.WAVE_M)
    assert (ap.WAVE_M, ap.WAVE_N, ap.MV_LONG) == (700, 357, 64) and list(np.diff(csc[0])) == lengths
    assert set(lengths) == {0, 1, 63, 64, 65, 127, 128, 129, 192, 700}
    long_lanes = [[j - w for j in range(w, min(w + 64, ap.WAVE_N)) if lengths[j] > 64] for w in range(0, ap.WAVE_N, 64)]
    assert long_lanes == [[], [0], [5, 20, 63], [1, 2], [], [36]]
    assert ap.WAVE_N - 5 * 64 == 37 and lengths[-1] == 65 and set(lengths[256:320]) == {64}
    x = ap.wave_x()
    assert np.isinf(x[10]) and np.isnan(x[20]) and np.count_nonzero(~np.isfinite(x)) == 2
    stores = [set(csc[1][csc[0][j] - 1:csc[0][j + 1] - 1] - 1) for j in range(ap.WAVE_N)]
    for r in (10, 20):
        hit = [r in s for s in stores]
        assert any(hit) and not all(h for h, l in zip(hit, lengths) if l > 0)        # only some columns store the row
    r = linalg.mul_transpose(csc, x)
    assert np.isnan(r).any() and np.isfinite(r).any() and np.count_nonzero(r[np.isfinite(r)]) > 100


def test_new_stars_and_the_prolongation_hub_column(orc, tmp_path_factory):
    model = am.Model(tmp_path_factory.mktemp("edge_amg_model"))

    def fd(*dims):
        O = orc.fdrand(*dims, rand_mode=1, seed=7, style=orc.KIND_UPDATE)       # (O owns what sparse() views)
        return tuple(np.array(a) for a in O.sparse().arrays())
    g = am.graphs(fd)
    assert list(g) == am.GRAPH_NAMES and {"star31", "star32", "star63"} <= set(am.GRAPH_NAMES)
    hub = {}
    for deg in (31, 32, 63, 64):
        csc, theta = g["star%d" % deg]
        assert np.diff(csc[0]).max() == deg + 1                                       # the hub column of A
        with np.errstate(all="ignore"):
            M = am.AMGModel(model, csc, max_coarse=1, theta=theta)
        assert [L.n for L in M.levels] == [deg + 1, 1]
        P = M.levels[0].P
        assert len(P[0]) == 2                                                         # one aggregate: P's only column is the hub's
        hub[deg] = int(P[0][1] - P[0][0])
        u = M.ldiv(np.random.default_rng(deg).standard_normal(deg + 1))
        assert np.isfinite(u).all() and np.any(u != 0.0)
    assert hub == {31: 32, 32: 33, 63: 64, 64: 65}                                    # AMG_LONG at 32 | 33, AMG_TLONG at 64 | 65


def test_reduction_vectors():
    from test_linalg_gpu import NORM_P, close
    assert ap.RED_SIZES == [65537, 262144, 262145, 524289]
    assert ap.RED_GRID * ap.RED_MT + 1 == 262145 and 256 * ap.RED_MT + 1 == 65537 and ap.MAX_GRID * 256 + 1 == ap.GRID_N == 524289
    for N in ap.RED_SIZES:
        G = min(ap.RED_GRID, -(-N // ap.RED_MT))
        sp_ = ap.reduction_specials(N)
        if N == 65537:
            assert G == 257 and sp_ == [256 * ap.RED_MT]                              # the 257th partial holds this element alone
        if N >= 262145:
            assert G == 1024 and sp_[0] == G * ap.RED_MT                              # the first element of the second round
        if N == 524289:
            assert sp_[-1] == 2 * G * ap.RED_MT and sp_[1] == sp_[-1] - 1             # the second round's last, the third's only
        for negative in (False, True):
            v = ap.reduction_vector(N, negative)
            rest = np.delete(np.abs(v), sp_)
            assert len(v) == N and rest.min() >= 0.5 and rest.max() <= 1.5
            for p in NORM_P:
                if (p < 0) != negative:
                    continue
                want = linalg_modellib.norm_ref(v, p)
                assert math.isfinite(want) and want > 0
                for i in sp_:                                                         # the reference without that element
                    if math.isinf(p) and i != sp_[-1]:
                        continue                                                      # (max / min: the extreme one is the last)
                    assert not close(linalg_modellib.norm_ref(np.delete(v, i), p), want), (N, p, i)


def test_grid_matrix(linalg):
    csc, n = ap.grid_matrix()
    cp, rv, nz = csc
    assert n == 524289 and len(rv) == 2 * n and np.all(np.diff(cp) == 2)
    assert np.all(np.diff(rv.reshape(n, 2), axis=1) > 0)
    rows = np.bincount(rv - 1, minlength=n)
    assert rows[n - 1] == 33 and np.delete(rows, n - 1).max() <= 3                    # the transpose's only long column: 32 | 33
    colsum = np.abs(nz).reshape(n, 2).sum(axis=1)
    rowsum = np.bincount(rv - 1, weights=np.abs(nz), minlength=n)
    assert int(np.argmax(colsum)) == n - 1 and np.sort(colsum)[-2] < colsum[n - 1] - 1
    assert int(np.argmax(rowsum)) == n - 1 and np.sort(rowsum)[-2] < rowsum[n - 1] - 1
    assert (n - 1) // 256 == ap.MAX_GRID                                              # segment n-1 is workgroup 0's second round
    assert linalg.opnorm_general(n, csc, 1) == colsum[n - 1] and linalg.opnorm_general(n, csc, math.inf) > 20


def test_frontier(tmp_path_factory):
    model = iluk_modellib.Model(tmp_path_factory.mktemp("edge_iluk_model"))
    assert ap.SHORT_COL == 16
    for width in (16, 17):
        csc, tcsc, r1, r2 = ap.frontier(width)
        n, src, u1, u2 = ap.FRONTIER_N, ap.FRONTIER_SOURCE, ap.FRONTIER_U1, ap.FRONTIER_U2
        check_csc(csc, n)
        check_csc(tcsc, n)
        lens = np.diff(csc[0])
        assert lens[u1] == width and lens[u2] == width and u1 < u2 < src
        assert np.delete(lens, [u1, u2]).max() <= 2                                   # every other frontier vertex is short
        assert r1.min() > src and r2.min() > src and len(set(r2) - set(r1)) == width - 1 - (width - 1) // 2 > 0
        back = ap.transpose_csc(n, tcsc)
        assert all(np.array_equal(a, b) for a, b in zip(back, csc))
        for K, want1, want2 in ((0, 0, 0), (1, width - 2, 0), (2, width - 2, len(set(r2) - set(r1))), (3, width - 2, len(set(r2) - set(r1)))):
            for which, arrays in (("lower", csc), ("upper", tcsc)):
                P = model.precon(arrays, K)
                lev = iluk_modellib.levels_as_dict(P.B, P.lev)
                mine = {k: l for k, l in lev.items() if (k[1] if which == "lower" else k[0]) == src
                        and (k[0] if which == "lower" else k[1]) > src}
                assert sum(l == 1 for l in mine.values()) == want1 and sum(l == 2 for l in mine.values()) == want2, (width, K, which)
                _, vl, vu = iluk_modellib.parallel_levels(arrays[0], arrays[1], K)
                assert max(vl + vu) <= 64                                             # the wave form serves every column
                u = P.ldiv(np.ones(n))
                assert np.isfinite(u).all() and np.any(u != 0.0)


# =================================================================================================================================
# the factorization side: tests/factor_patterns.py
# =================================================================================================================================
import factor_patterns as fp  # noqa: E402
import lu_modellib  # noqa: E402


def factor_csc(case):
    """the CSC arrays of a factor_patterns case, after the checks every case must pass: unique triplets in range, off-diagonals in
    (-1, 1), every diagonal 1 + max(row abs sum, column abs sum)"""
    I, J, V, n = case
    assert len(I) == len(J) == len(V) and len(np.unique((I - 1) * n + (J - 1))) == len(I)
    assert I.min() >= 1 and I.max() <= n and J.min() >= 1 and J.max() <= n
    assert np.all(np.abs(V[I != J]) < 1.0)
    arrays = ep.csc_arrays(n, I, J, V)
    S = sp.csc_matrix((arrays[2], arrays[1] - 1, arrays[0] - 1), shape=(n, n))
    d = S.diagonal()
    rows = np.asarray(abs(S).sum(axis=1)).ravel() - d
    cols = np.asarray(abs(S).sum(axis=0)).ravel() - d
    np.testing.assert_allclose(d, 1.0 + np.maximum(rows, cols), rtol=1e-13, atol=0)
    return arrays


def automatic_wave(arrays):
    """iluam_update's automatic rule"""
    return len(arrays[1]) >= fp.FW_MIN_AVG * (len(arrays[0]) - 1)


def factor_widths(arrays):
    return ep.widths_of(level_schedules(arrays[0], arrays[1])[0])


def test_factor_constants():
    assert (fp.FW_ROWS, fp.FW_MIN_AVG, fp.WAVE, fp.LT, fp.AMG_LONG) == (2048, 24, 64, 256, 32) and fp.LT == ep.LT


def test_exact_nnz_sits_on_the_switch(model):
    n = 100
    on, below = fp.exact_nnz(n, 24 * n, seed=5), fp.exact_nnz(n, 24 * n - 1, seed=5)
    a, b = factor_csc(on), factor_csc(below)
    assert len(a[1]) == 2400 == fp.FW_MIN_AVG * n and len(b[1]) == 2399
    assert automatic_wave(a) and not automatic_wave(b)
    # the second is the first minus its last off-diagonal entry
    assert np.array_equal(on[0][n:-1], below[0][n:]) and np.array_equal(on[1][n:-1], below[1][n:]) and np.array_equal(on[2][n:-1], below[2][n:])
    for arrays in (a, b):
        assert np.all(np.diff(arrays[0]) >= 1) and np.isfinite(model.factor(arrays)[0]).all()


@pytest.mark.parametrize("n,nnz", [(2047, 55087), (2048, 55114), (2049, 55141)])
def test_arrowband_columns_at_the_staging_edge(model, n, nnz):
    case = fp.arrowband(n)
    arrays = factor_csc(case)
    cp, rv, _ = arrays
    lens = np.diff(cp)
    assert len(rv) == nnz == 27 * n - 182 and automatic_wave(arrays) and fp.FW_MIN_AVG * n == {2047: 49128, 2048: 49152, 2049: 49176}[n]
    assert int(lens.argmax()) == n - 1 and lens[n - 1] == n and np.delete(lens, n - 1).max() == 26
    assert (lens[n - 1] <= fp.FW_ROWS) == (n <= 2048)                       # two staged sizes and the first unstaged one
    assert np.all(rv[cp[1:n] - 2] == n)                                    # every other column ends with the last row ...
    hit, inside, beyond = fp.search_outcomes(cp, rv)
    assert hit > 0 and beyond == 0                                         # ... so no search runs beyond a column's end
    assert factor_widths(arrays) == [1] * n                                 # n levels of one column
    f, diag = model.factor(arrays)
    assert np.isfinite(f).all()
    assert np.isfinite(model.ldiv(arrays, f, diag, np.ones(n))).all()
    t = factor_csc(fp.transposed(case))                                     # the transpose: the same pattern, other values
    assert np.array_equal(t[0], cp) and np.array_equal(t[1], rv) and not np.array_equal(t[2], arrays[2])
    assert np.isfinite(model.factor(t)[0]).all()


def test_arrowband_with_the_long_column_in_the_middle(model):
    n, hub = 2049, 1024
    arrays = factor_csc(fp.arrowband(n, hub=hub))
    cp, rv, _ = arrays
    lens = np.diff(cp)
    assert int(lens.argmax()) == hub != n - 1 and lens[hub] == n > fp.FW_ROWS and np.delete(lens, hub).max() == 26
    assert automatic_wave(arrays) and len(rv) == 55141
    # the columns behind the hub store row `hub` above their diagonal: they read the long column as their column i, whose rows below
    # its diagonal take (n - 1 - hub) / 64 = 16 rounds of the lane stride
    assert all(hub + 1 in rv[cp[j] - 1:cp[j + 1] - 1] for j in range(hub + 1, n)) and (n - 1 - hub) == 16 * fp.WAVE
    base = ep.csc_arrays(n, *fp.arrowband(n)[:3])
    inv = np.concatenate([np.arange(hub), [n - 1], np.arange(hub, n - 1)])   # new index -> old index
    B = sp.csc_matrix((np.ones(len(base[1])), base[1] - 1, base[0] - 1), shape=(n, n))[inv][:, inv]
    M = sp.csc_matrix((np.ones(len(rv)), rv - 1, cp - 1), shape=(n, n))
    assert (B != M).nnz == 0                                                # a symmetric permutation of arrowband(n)
    hit, inside, beyond = fp.search_outcomes(cp, rv)
    assert hit > 0 and inside > 0 and beyond > 0
    assert np.isfinite(model.factor(arrays)[0]).all()


@pytest.mark.parametrize("copies,launches", [(5, (0, 1)), (256, (0, 25)), (257, (25, 0)), (258, (25, 0)), (259, (25, 0)), (260, (25, 0))])
def test_cliques_level_widths_and_launches(copies, launches):
    """m = 25 levels of `copies` columns: one thin launch (5: wave 0 takes members 0 and 4), a thin launch per level (256: 64 members
    per wave), wide launches whose last workgroup has copies - 256 = 1, 2, 3, 4 live waves"""
    arrays = factor_csc(fp.cliques(copies, 25))
    assert np.all(np.diff(arrays[0]) == 25) and len(arrays[1]) == 625 * copies and automatic_wave(arrays)
    widths = factor_widths(arrays)
    assert widths == [copies] * 25 and ep.launch_list(widths) == launches
    if copies > fp.LT:
        per_group = fp.LT // fp.WAVE
        assert copies - (copies - 1) // per_group * per_group == copies - 256
    if copies == 260:
        assert (len(arrays[0]) - 1, len(arrays[1])) == (6500, 162500)


@pytest.mark.parametrize("m,rounds", [(64, 1), (65, 1), (66, 2), (131, 3)])
def test_single_clique_rows_below_the_first_diagonal(model, m, rounds):
    arrays = factor_csc(fp.cliques(1, m))
    cp, rv, _ = arrays
    below = int((rv[cp[0] - 1:cp[1] - 1] > 1).sum())
    assert below == m - 1 and -(-below // fp.WAVE) == rounds and automatic_wave(arrays)
    assert factor_widths(arrays) == [1] * m
    assert np.isfinite(model.factor(arrays)[0]).all()


def test_sparse_dense_enough_search_outcomes(model):
    arrays = factor_csc(fp.sparse_dense_enough(seed=3))
    cp, rv, nz = arrays
    assert len(rv) == 9270 >= fp.FW_MIN_AVG * 300 == 7200 and automatic_wave(arrays)
    S = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(300, 300))
    assert ((S != 0) != (S != 0).T).nnz > 0                                 # non-symmetric
    hit, inside, beyond = fp.search_outcomes(cp, rv)
    print("hits %d, misses inside column j %d, beyond its last row %d" % (hit, inside, beyond))
    assert (hit, inside, beyond) == (9404, 76903, 3719) and min(hit, inside, beyond) > 0
    assert np.isfinite(model.factor(arrays)[0]).all()


def test_search_outcomes_by_hand():
    """column 2 = rows {0, 2, 5}, column 0 = rows {0, 1, 2, 4, 9} (0-based): from v = 0 of column 2, row 1 falls before row 2 and
    row 4 between rows 2 and 5 (inside), row 2 hits, row 9 lies beyond the last row"""
    n = 10
    I = np.concatenate([np.arange(n), [1, 2, 4, 9, 0, 5]])
    J = np.concatenate([np.arange(n), [0, 0, 0, 0, 2, 2]])
    cp, rv, _ = ep.csc_arrays(n, I + 1, J + 1, np.ones(len(I)))
    assert fp.search_outcomes(cp, rv) == (1, 2, 1)


def test_forced_cases_need_the_hook():
    """the layered patterns of the launch-list tests hold 3-5 entries per column: only the hook brings them to the wave form"""
    for name in sorted(ep.WIDTHS):
        for form in ("upper", "symmetric"):
            I, J, V, n = ep.layered(ep.WIDTHS[name], form, seed=3)
            assert len(I) < fp.FW_MIN_AVG * n and len(I) <= 5 * n
            assert 0 in ep.PRESCRIBED[form]


@pytest.mark.parametrize("hubs,entries,by", fp.MULTI_HUB_CASES)
def test_multi_hub_long_vertices(hubs, entries, by):
    n = fp.MULTI_HUB_N
    arrays = factor_csc(fp.multi_hub(n, hubs, entries, by))
    cp, rv, _ = arrays
    bycol, byrow = fp.long_vertices(cp, rv)
    assert list(bycol) == (hubs if by in ("col", "both") else []) and list(byrow) == (hubs if by in ("row", "both") else [])
    percol, perrow = np.diff(cp), np.bincount(rv - 1, minlength=n)
    for h in hubs:
        path = 2 - (h in (0, n - 1))
        assert percol[h] == 1 + path + (entries if by != "row" else 0) and perrow[h] == 1 + path + (entries if by != "col" else 0)
    others = np.setdiff1d(np.arange(n), hubs)
    assert max(percol[others].max(), perrow[others].max()) <= 3 + len(hubs) <= fp.AMG_LONG
    S = sp.csc_matrix((np.ones(len(rv)), rv - 1, cp - 1), shape=(n, n))
    assert sp.csgraph.connected_components(S, directed=False)[0] == 1


def test_multi_hub_lanes():
    """which lanes of which waves fold: lane 0, lane 63, both, two neighbours, three in wave 1, lane 43 of the ragged wave 4"""
    n = fp.MULTI_HUB_N
    assert n == 300 and n - 4 * fp.WAVE == 44 and (n - 1) // fp.LT == 1
    where = [[(h // fp.WAVE, h % fp.WAVE) for h in hubs] for hubs in fp.HUB_SETS]
    assert where == [[(0, 0)], [(0, 63)], [(0, 0), (0, 63)], [(0, 10), (0, 11)], [(1, 0), (1, 36), (1, 63)], [(4, 43)]]
    assert len(fp.MULTI_HUB_CASES) == 14
    assert {(e, by) for _, e, by in fp.MULTI_HUB_CASES} == {(33, "col"), (65, "row"), (33, "both"), (65, "both")}
    assert 33 == fp.AMG_LONG + 1 and 65 == fp.WAVE + 1                     # one and two rounds of the fold


def test_clique_components_node_sizes(tmp_path_factory):
    """what the LU model makes of them with leaf_size 70.  Separate cliques of 63, 64, 65: three dense leaves of exactly those sizes,
    no struct.  With a path of 10 behind each the separator is a vertex of the path (the middle level set of the search), and the
    leaf beside it holds the clique and the three path vertices next to it: nodes of 66, 67, 68 for cliques of 63, 64, 65.  Cliques of
    59, 60, 61 with a path of 12 (four path vertices stay with the clique) give nodes of exactly 63, 64, 65 -- each with the separator
    as its struct, so the separator's column lists a node of that size"""
    lm = lu_modellib.Model(tmp_path_factory.mktemp("edge_lu_model"))

    def nodes(sizes, tail):
        arrays = factor_csc(fp.clique_components(sizes, tail))
        F = lm.lu(arrays, 70)
        bcp, brv, _ = F.B
        out = []
        for s in np.unique(F.nstart):
            struct = int((brv[bcp[s] - 1:bcp[s + 1] - 1] - 1 >= s + F.nsize[s]).sum())
            out.append((int(F.nsize[s]), struct))
        assert np.isfinite(F.fval).all()
        return out, F.stats

    got, st = nodes([63, 64, 65], 0)
    assert got == [(63, 0), (64, 0), (65, 0)] and (st["rounds"], st["nodes"], st["largest_node"]) == (1, 3, 65)
    got, st = nodes([63, 64, 65], 10)
    assert [g for g in got if g[0] > 60] == [(66, 1), (67, 1), (68, 1)] and st["rounds"] == 2
    got, st = nodes(*fp.CLIQUE_TAILS_AT_THE_EDGE)
    assert [g for g in got if g[0] > 59] == [(63, 1), (64, 1), (65, 1)] and st["rounds"] == 2
    assert sorted(g for g in got if g[0] <= 59) == [(1, 0)] * 3 + [(7, 1)] * 3   # the separators and the far ends of the paths


# =================================================================================================================================
# the approximate-inverse and threshold side: tests/approx_patterns.py
# =================================================================================================================================
import os  # noqa: E402

import approx_patterns as xp  # noqa: E402
import ilut_modellib  # noqa: E402
import spai_modellib  # noqa: E402


@pytest.fixture(scope="module")
def spai(tmp_path_factory):
    return spai_modellib.Model(tmp_path_factory.mktemp("edge_spai_model"))


@pytest.fixture(scope="module")
def ilut(tmp_path_factory):
    return ilut_modellib.Model(tmp_path_factory.mktemp("edge_ilut_model"))


def spai_limits(esp):
    return esp._lib.ESP_SPAI_WAVE_DOUBLES, esp._lib.ESP_SPAI_DENSE_MAX


def named_tier(esp, csc, k=0):
    p, q, tc, maxlen = xp.column_sizes(csc, k)
    return (p, q, tc), xp.spai_tier(p, q, tc, maxlen, *spai_limits(esp))


def lstsq_error(csc, m, columns):
    """the largest |m - m_ref|_inf / max(1, |m_ref|_inf) over `columns`, m_ref by numpy.linalg.lstsq on the same I and J, and the
    largest condition number of a B"""
    cp, rv, nz = csc
    n = len(cp) - 1
    A = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))
    worst, cond = 0.0, 0.0
    for k in columns:
        J = rv[cp[k] - 1:cp[k + 1] - 1] - 1
        I = np.unique(np.concatenate([rv[cp[j] - 1:cp[j + 1] - 1] - 1 for j in J]))
        B = A[I][:, J].toarray()
        ref = np.linalg.lstsq(B, (I == k).astype(np.float64), rcond=None)[0]
        got = m[cp[k] - 1:cp[k + 1] - 1]
        worst = max(worst, float(np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(ref)))))
        cond = max(cond, float(np.linalg.cond(B)))
    return worst, cond


def test_approx_constants(esp):
    W, D = spai_limits(esp)
    assert (W, D, xp.SORT_MAX, xp.SIZE_WAVE, xp.GRID_MAX, xp.RGRID) == (512, 12288, 16384, 512, 1 << 20, 1024)
    assert 22 * 22 <= W < 23 * 23 and 110 * 110 <= D < 111 * 111 and 128 * 128 == xp.SORT_MAX < 129 * 129
    # (the three are not exported: tied to the source, whatever its spacing)
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "extendablesparse.jl_amd", "csrc", "spai.hip")).read()
    for pattern in (r"SORT_MAX\s*=\s*16384\s*;", r"GRID_MAX\s*=\s*1u\s*<<\s*20\s*;",
                    r"min<i64>\(\s*stats\[3\]\s*,\s*1024\s*\)\s*,\s*\(\s*\(i64\)\s*1\s*<<\s*27\s*\)\s*/\s*rslot"):
        assert re.search(pattern, text), pattern
    assert xp.R_DOUBLES == 1 << 27


@pytest.mark.parametrize("m,tier", [(22, xp.TIER_WAVE), (23, xp.TIER_WIDE), (110, xp.TIER_WIDE)])
def test_dense_block_accepted(esp, spai, m, tier):
    """p = q = m and tc = m * m in every column; 22: the wave form's sort full (484 of 512 words, no wide column), 23: q q > 512 and
    tc > 512; 110: 12100 <= 12288 doubles, 16384 padded words of sort.  Every column against lstsq"""
    csc = xp.dense_block(m)
    for k in (0, m // 2, m - 1):
        assert named_tier(esp, csc, k) == ((m, m, m * m), (tier, m))
    assert xp.size_form(m * m) == ("wave" if m == 22 else "group")
    assert 1 << (m * m - 1).bit_length() == {22: 512, 23: 1024, 110: 16384}[m]
    vals, pcol, stats = spai.spai1(csc)
    assert np.all(pcol == m) and stats == (m, m, m * m)
    err, cond = lstsq_error(csc, vals, range(m))
    print("dense_block(%d): model against lstsq %.3e, cond(B) %.3f" % (m, err, cond))
    assert err <= 1e-10, (err, cond)


@pytest.mark.parametrize("m,tier,p", [(111, xp.TIER_REFUSED, 111), (128, xp.TIER_REFUSED, 128), (129, xp.TIER_REFUSED_BOUND, 129)])
def test_dense_block_refused(esp, m, tier, p):
    """tc = 12321 and 16384 are sorted and refused with p; 16641 > SORT_MAX is refused unsorted with the bound
    max(maxlen, ceil(tc / q)) = 129"""
    csc = xp.dense_block(m)
    assert named_tier(esp, csc, 0) == ((m, m, m * m), (tier, p))
    assert (m * m > xp.SORT_MAX) == (tier == xp.TIER_REFUSED_BOUND) and m * m > spai_limits(esp)[1]


@pytest.mark.parametrize("p,q,tier,form", [(64, 8, xp.TIER_WAVE, "wave"), (57, 9, xp.TIER_WIDE, "group")])
def test_full_lists(esp, spai, p, q, tier, form):
    """test_tier_boundary's (p, q) with tc = p q: 512 is the wave form's last size, 513 the workgroup form's first"""
    csc = xp.full_lists(p, q)
    assert named_tier(esp, csc, 0) == ((p, q, p * q), (tier, p)) and xp.size_form(p * q) == form
    assert xp.diagonal_position(csc, 0) == -1 and 1 in csc[1][csc[0][1] - 1:csc[0][2] - 1]        # row 0 is in I
    for k in range(1, q + 1):                                  # the q columns: p unknowns over p rows, the workgroup tier's
        assert named_tier(esp, csc, k) == ((p, p, q + q * p + (p - q - 1)), (xp.TIER_WIDE, p))
    vals, pcol, stats = spai.spai1(csc)
    assert pcol[0] == p and stats == (p, p, p * p)
    err, cond = lstsq_error(csc, vals, [0])
    print("full_lists(%d, %d): model against lstsq %.3e, cond(B) %.3f" % (p, q, err, cond))
    assert err <= 1e-10 and np.abs(vals[:q]).max() > 0.0, (err, cond)


@pytest.mark.parametrize("p,q", [(768, 16), (128, 96)])
def test_sized_at_the_cap(esp, spai, p, q):
    """p q = ESP_SPAI_DENSE_MAX exactly, tc = p + q - 1; every column against lstsq"""
    csc = xp.sized(p, q)
    assert p * q == spai_limits(esp)[1]
    assert named_tier(esp, csc, 0) == ((p, q, p + q - 1), (xp.TIER_WIDE, p))
    ps, qs, tcs = xp.all_sizes(csc)
    assert (ps * qs).max() == p * q and int((ps * qs).argmax()) == 0 and ps[0] == p and tcs[0] == p + q - 1
    vals, pcol, stats = spai.spai1(csc)
    assert np.array_equal(pcol, ps) and stats == (p, max(q, int(qs.max())), p * q)
    err, cond = lstsq_error(csc, vals, range(p))
    print("sized(%d, %d): model against lstsq %.3e, cond(B) %.3f" % (p, q, err, cond))
    assert err <= 1e-10, (err, cond)


def fan_tiers(esp, p, q, shared=False):
    """the sizes and tiers of fan(p, q): column 0, and the q columns of its unknowns"""
    csc = xp.fan(p, q, shared)
    assert p * q == spai_limits(esp)[1]
    assert named_tier(esp, csc, 0) == ((p, q, p * q if shared else p), (xp.TIER_WIDE, p))
    for k in range(1, q + 1):
        own = p if shared else k * p // q - (k - 1) * p // q                    # the column's unknowns
        seen = q if shared or k == 1 else 0                                   # column 0 is the only one of them that stores rows
        assert named_tier(esp, csc, k) == ((seen, own, seen), (xp.TIER_WIDE, seen))
    return csc


@pytest.mark.parametrize("p,q,shared", [(1536, 8, False), (1536, 8, True), (4096, 3, False), (6144, 2, False)])
def test_fan_at_the_cap(esp, spai, p, q, shared):
    """p q = ESP_SPAI_DENSE_MAX with p / q = 192, 1365 and 3072 (24, 64 and 96 lane strides): only columns without a diagonal over
    empty columns allow it (a column of len rows that stores its diagonal has a problem of len * len doubles at least).  (1536, 8)
    with all eight lists full: tc = 12288 = ESP_SPAI_DENSE_MAX exactly, what spai1_k's `fits` compares, every row eight times in
    a sort of 16384 padded words.  Column 0 against lstsq"""
    csc = fan_tiers(esp, p, q, shared)
    with np.errstate(all="ignore"):
        vals, pcol, stats = spai.spai1(csc)
    assert pcol[0] == p and stats == (p, p if shared else -(-p // q), p * q)
    err, cond = lstsq_error(csc, vals, [0])
    print("fan(%d, %d%s): model against lstsq %.3e, cond(B) %.3f" % (p, q, ", shared" if shared else "", err, cond))
    assert err <= 1e-10 and np.all(np.isfinite(vals[:q])) and np.abs(vals[:q]).max() > 0.0


def test_one_unknown_at_the_cap(esp, spai):
    """(p, q) = (12288, 1): I full, tc = p = ESP_SPAI_DENSE_MAX, 192 lane strides, no column d > c; the model against the closed form
    m = b_0 / (b . b).  The column that the unknown names holds 12288 rows, so its own problem has 12288 unknowns over one row
    (accepted: 12288 doubles): 75 million ordered sums, most of this test's eight seconds"""
    p = 12288
    csc = fan_tiers(esp, p, 1)
    with np.errstate(all="ignore"):
        vals, pcol, stats = spai.spai1(csc)
    assert (pcol[0], pcol[1]) == (p, 1) and stats == (p, p, p)
    b = csc[2][csc[0][1] - 1:csc[0][2] - 1]
    ref = b[0] / np.dot(b, b)
    err = abs(vals[0] - ref) / max(1.0, abs(ref))
    print("fan(12288, 1): model against the closed form %.3e" % err)
    assert err <= 1e-10 and vals[0] != 0.0


def test_r_slots():
    """the second term of the launch's grid: 1 GiB of R slots"""
    assert xp.r_slots(1030, 40) == 1024 and xp.r_slots(110, 110) == 110
    assert xp.r_slots(9, 192) == 9 and xp.r_slots(9, 1536) == 9 and xp.r_slots(4, 1366) == 4 and xp.r_slots(3, 3072) == 3
    assert xp.r_slots(57, 1536) == 56 and xp.r_slots(2, 12288) == 1


@pytest.mark.parametrize("h,wide", [(22, 0), (23, 1)])
def test_hubs_on_the_qq_rule(esp, h, wide):
    """p q = 3 h <= 69: the q q rule alone decides"""
    csc = xp.hub(h)
    want = xp.TIER_WIDE if wide else xp.TIER_WAVE
    assert named_tier(esp, csc, 0) == ((3, h, h + 2), (want, 3)) and 3 * h <= spai_limits(esp)[0]
    assert (h * h > spai_limits(esp)[0]) == bool(wide)
    for k in range(1, h + 1):
        assert named_tier(esp, csc, k)[1][0] == xp.TIER_WAVE


def test_many_wide(esp):
    csc = xp.many_wide(1030)
    n = len(csc[0]) - 1
    assert n == 515 * 24 + 515 * 41 == 33475
    ps, qs, tcs = xp.all_sizes(csc)
    W, D = spai_limits(esp)
    wide = (ps * qs > W) | (qs * qs > W)
    assert int(wide.sum()) == 1030 > xp.RGRID and (ps * qs).max() <= D and tcs.max() <= xp.SIZE_WAVE
    assert sorted(set(qs[wide])) == [23, 40] and np.all(ps[wide] == 3)
    listed = np.flatnonzero(wide)
    assert qs[listed[0]] == 23 and qs[listed[1]] == 40 and qs[listed[1024]] == 23 and qs[listed[1025]] == 40
    assert (int(ps.max()), int(qs.max()), int((ps * qs).max())) == (41, 40, 123)


def test_tridiagonal_past_the_grid(spai):
    n = xp.GRID_MAX + 1
    csc = xp.tridiagonal(n)
    cp, rv, nz = csc
    assert len(rv) == 3 * n - 2 and np.array_equal(np.diff(cp)[[0, 1, n - 1]], [2, 3, 2])
    assert np.array_equal(rv[:5], [1, 2, 1, 2, 3]) and np.array_equal(rv[-2:], [n - 1, n])
    assert xp.column_sizes(csc, n - 1) == (3, 2, 5, 3) and xp.column_sizes(csc, 5) == (5, 3, 9, 3)
    small = xp.tridiagonal(40)
    vals, pcol, stats = spai.spai1(small)
    assert stats == (5, 3, 15)
    assert lstsq_error(small, vals, range(40))[0] <= 1e-10


def test_spai0_columns(spai):
    csc = xp.spai0_matrix()
    cp, rv, nz = csc
    n = len(cp) - 1
    assert n == xp.SPAI0_N and n % 4 == 3
    lens = np.diff(cp)
    assert [int(lens[j]) for j in sorted(xp.SPAI0_COLUMNS)] == [63, 64, 65, 130, 200, 200, 130, 0]
    pos = {j: xp.diagonal_position(csc, j) for j in xp.SPAI0_COLUMNS}
    assert pos == {5: 5, 70: 63, 100: 64, 150: 129, 160: 160, 180: -1, 190: 109, 200: -1}
    assert pos[150] == lens[150] - 1 and pos[150] // xp.WAVE == 2 and pos[100] // xp.WAVE == 1 and pos[190] // xp.WAVE == 1
    with np.errstate(all="ignore"):
        d = spai.spai0(csc)
        s = spai.spai0(xp.spai0_matrix(special=True))
    A = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n)).toarray()
    keep = np.ones(n, bool)
    keep[[180, 200]] = False
    assert np.allclose(d[keep], np.diag(A)[keep] / (A * A).sum(0)[keep], rtol=1e-14, atol=0.0)
    assert bits(d[180:181])[0] == 0 and np.isnan(d[200])
    assert np.isnan(s[160]) and s[150] == 0.0 and np.array_equal(np.isfinite(s), np.isfinite(d) & (np.arange(n) != 160))


COMBS = [(200, 12), (300, 12), (4200, 12)]


@pytest.mark.parametrize("up,L", COMBS)
def test_comb_reaches_every_end_of_the_lookup(esp, ilut, up, L):
    csc, j = xp.comb(up, L)
    cp, rv, nz = csc
    n = len(cp) - 1
    ups = xp.upper_counts(csc)
    assert ups[j] == up and 8 * L < up and np.delete(ups, j).max() == 1
    Wv, G = esp._lib.ESP_ILUT_WAVE_UPPER, esp._lib.ESP_ILUT_GROUP_UPPER
    assert (up <= Wv, Wv < up <= G, up > G) == {200: (True, False, False), 300: (False, True, False), 4200: (False, False, True)}[up]
    rows = rv[cp[j] - 1:cp[j + 1] - 1] - 1
    K = rows[:up]
    assert j - K.max() - 1 >= 40 and np.all(np.diff(K) == 2)
    perrow = np.bincount(rv - 1, minlength=n)
    assert np.all(perrow[rows[rows != j]] == L)
    S = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))
    d = S.diagonal()
    assert np.all(d > np.asarray(abs(S).sum(axis=0)).ravel() - d) and np.all(d > np.asarray(abs(S).sum(axis=1)).ravel() - d)
    out = xp.sweep_outcomes(csc)
    print("comb(%d, %d): n = %d, nnz = %d, %s" % (up, L, n, len(rv), out))
    assert min(out["hit"], out["miss"], out["exhausted"], out["bound"], out["carried"]) >= 16 and out["merge"] > 0
    assert out["lookup"] == len(rows) and out["merge"] == len(rv) - len(rows)
    for par in ((0.0, 0, 1), (1e-3, 1, 2)):
        P = ilut.precon(csc, *par)
        assert np.isfinite(P.F).all()
        got = xp.upper_counts((P.S[0], P.S[1]))
        assert got[j] == up if par[0] == 0.0 else up - 8 <= got[j] <= up      # (the drop rule takes an entry or two of the long column)
        tier = lambda u: int(u > Wv) + int(u > G)      # noqa: E731
        assert tier(got[j]) == tier(up) and np.delete(got, j).max() <= Wv


@pytest.mark.parametrize("L", [5, 31])
def test_switch_pair_sits_on_the_switch(esp, L):
    (a, ja), (b, jb) = xp.switch_pair(L)
    for (csc, j), up, look in ((a, ja), 8 * L, False), ((b, jb), 8 * L + 1, True):
        cp, rv, _ = csc
        n = len(cp) - 1
        assert xp.upper_counts(csc)[j] == up <= esp._lib.ESP_ILUT_WAVE_UPPER
        rows = rv[cp[j] - 1:cp[j + 1] - 1] - 1
        perrow = np.bincount(rv - 1, minlength=n)
        assert np.all(perrow[rows[rows != j]] == L) and perrow[j] == 2
        assert np.all((perrow[rows[rows != j]] * 8 < up) == look)
        out = xp.sweep_outcomes(csc)
        assert out["lookup"] == (len(rows) if look else 1)        # (row j itself holds two entries: always the look-up, ended at once)
        if look:
            assert min(out["hit"], out["miss"], out["exhausted"], out["bound"]) >= 16


@pytest.mark.parametrize("name", ["comb200", "comb300", "pair5a", "pair5b", "pair31a", "pair31b"])
def test_ilut_model_against_the_dense_restatement_on_the_combs(ilut, name):
    """test_ilut_model.py's comparison and bound (the patterns equal, the values to 1e-12 of the largest entry) on the look-up
    patterns: no sum holds more than L - 3 products here"""
    csc = {"comb200": lambda: xp.comb(200, 12), "comb300": lambda: xp.comb(300, 12), "pair5a": lambda: xp.switch_pair(5)[0],
           "pair5b": lambda: xp.switch_pair(5)[1], "pair31a": lambda: xp.switch_pair(31)[0], "pair31b": lambda: xp.switch_pair(31)[1]}[name]()[0]
    n = len(csc[0]) - 1
    worst = 0.0
    for tau, steps, sweeps in ((0.0, 0, 3), (1e-3, 1, 2)):
        P = ilut.precon(csc, tau, steps, sweeps, max_fill=1e6)
        Pd, Fd = ilut_modellib.dense_ilut(csc, tau, steps, sweeps)
        Pm, Fm = ilut_modellib.dense_from(P.S, P.F, n)
        assert np.array_equal(Pm, Pd), (name, tau, steps)
        err = np.abs(Fm - Fd).max() / np.abs(Fd).max()
        worst = max(worst, err)
        assert err <= 1e-12, (name, tau, steps, err)
    print("%s: model against the dense restatement %.3e" % (name, worst))
