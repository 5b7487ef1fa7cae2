"""CPU: the crafted patterns of tests/edge_patterns.py are what they claim to be -- the prescribed schedule of every layered
pattern has exactly the prescribed level widths (by iluam_modellib's NumPy restatement of the schedules), launch_list gives the
hand-written launch counts, the capacity matrix holds its table of per-block entry counts (counted with SciPy), and the C
models' factorizations and ldiv! on every pattern are finite."""
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
