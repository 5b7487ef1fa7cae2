"""CPU: the model of AMGPreconditioner (tests/amg_model.c through tests/amg_modellib.py) is held to account by its own properties
-- every node aggregated exactly once, roots pairwise further than two strong edges apart, aggregates of diameter <= 4, the
Gauss-Jordan inverse, a symmetric V-cycle for a symmetric matrix, the level sizes of a second, independent NumPy / SciPy
restatement -- and the new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path

import amg_modellib as am
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = am.EMPTY


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return am.Model(tmp_path_factory.mktemp("amg_model"))


def fdrand_csc(orc, *dims):
    O = orc.fdrand(*dims, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
    return tuple(np.array(a) for a in O.sparse().arrays())


def graphs(orc):
    g = am.graphs(lambda *dims: fdrand_csc(orc, *dims))
    assert list(g) == am.GRAPH_NAMES
    return g


def strong_graph(csc, strong):
    cp, rv, _ = csc
    n = len(cp) - 1
    cols = np.repeat(np.arange(n), np.diff(cp))
    keep = strong.astype(bool)
    return sp.csr_matrix((np.ones(int(keep.sum())), (rv[keep] - 1, cols[keep])), shape=(n, n))


def test_aggregation_properties(model, orc):
    for name, (csc, theta) in graphs(orc).items():
        n = len(csc[0]) - 1
        strong = model.strength(csc, theta)
        agg, nc, rounds, state = model.aggregate(csc, strong)
        if n == 0:
            assert nc == 0 and rounds == 0
            continue
        G = strong_graph(csc, strong)
        assert (G != G.T).nnz == 0, name                                   # the strength relation is symmetric
        assert rounds >= 1 and set(np.unique(state)) <= {1, 2}, name
        # every node is aggregated exactly once, every aggregate holds exactly one root, numbered in index order
        assert agg.min() >= 0 and agg.max() == nc - 1 and len(np.unique(agg)) == nc, name
        roots = np.flatnonzero(state == 1)
        assert len(roots) == nc and np.array_equal(agg[roots], np.arange(nc)), name
        # roots pairwise at strong-graph distance > 2; the set is maximal (everybody else within 2 of a root)
        G2 = sp.csr_matrix(G + G @ G)
        R = G2[roots][:, roots].tolil()
        R.setdiag(0)
        assert R.nnz == 0, name
        reach = np.asarray(G2[:, roots].sum(axis=1)).ravel() > 0
        reach[roots] = True
        assert reach.all(), name
        # every aggregate is connected inside itself with diameter <= 4
        for a in range(nc):
            mem = np.flatnonzero(agg == a)
            if len(mem) > 1:
                d = shortest_path(G[mem][:, mem], unweighted=True)
                assert np.isfinite(d).all() and d.max() <= 4, (name, a)
        # nodes without strong neighbours are singleton roots
        lonely = np.flatnonzero(np.asarray(G.sum(axis=1)).ravel() == 0)
        assert np.all(state[lonely] == 1), name


def test_theta_removes_edges_on_the_convection_diffusion_matrix(model):
    csc = am.convdiff(6, 5, 4, 4.0)
    cp, rv, _ = csc
    offdiag = int(np.sum(rv - 1 != np.repeat(np.arange(len(cp) - 1), np.diff(cp))))
    s0, s25 = model.strength(csc, 0.0), model.strength(csc, 0.25)
    assert int(s0.sum()) == offdiag                     # theta = 0: every non-zero off-diagonal pair
    assert 0 < int(s25.sum()) < offdiag                 # theta = 0.25 removes the weak (z) couplings ...
    assert model.aggregate(csc, s25)[1] > model.aggregate(csc, s0)[1]   # ... and the aggregates get smaller


def test_hash_and_strength_rules(model):
    # hash32 of the issue, restated: x = i + 1; x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
    def h32(i):
        x = (i + 1) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    # two nodes joined by one edge: the larger key becomes the root in round 1, the other one is excluded in round 2 and joins it
    agg, nc, rounds, state = model.aggregate(am.path_graph(2), model.strength(am.path_graph(2), 0.0))
    root = 0 if (h32(0) << 32 | 0) > (h32(1) << 32 | 1) else 1
    assert nc == 1 and rounds == 2 and state[root] == 1 and state[1 - root] == 2 and list(agg) == [0, 0]
    # a stored zero pair is no edge, one non-zero side is; a NaN loses against a number, two NaN are no edge; -0.0 is zero
    dense = np.array([[2.0, 0.0, 1.0, np.nan, 5.0], [0.0, 2.0, -0.0, 7.0, 5.0], [0.0, 3.0, 2.0, np.nan, 5.0],
                      [np.nan, np.nan, np.nan, 2.0, 5.0], [5.0, 5.0, 5.0, 5.0, 2.0]])
    n = 5
    cp = 1 + n * np.arange(n + 1, dtype=np.int64)
    rv = np.tile(np.arange(1, n + 1, dtype=np.int64), n)
    full = (cp, rv, np.ascontiguousarray(dense.T).reshape(-1))
    st = model.strength(full, 0.0).reshape(n, n).T     # st[i, j]
    want = np.array([[0, 0, 1, 0, 1], [0, 0, 1, 1, 1], [1, 1, 0, 0, 1], [0, 1, 0, 0, 1], [1, 1, 1, 1, 0]])
    assert np.array_equal(st, want)
    # theta: m*m >= theta^2*|a_ii|*|a_jj| exactly at the boundary
    two = (np.array([1, 3, 5]), np.array([1, 2, 1, 2]), np.array([4.0, -1.0, -0.5, 4.0]))
    assert model.strength(two, 0.25).tolist() == [0, 1, 1, 0]          # 1*1 >= (1/16)*16
    assert model.strength(two, 0.26).tolist() == [0, 0, 0, 0]
    assert model.check(two) == (0, 0)
    assert model.check((np.array([1, 2, 4]), np.array([1, 1, 2]), np.ones(3))) == (0, 2)      # (1,2) without (2,1)
    assert model.check((np.array([1, 3, 4]), np.array([1, 2, 1]), np.ones(3))) == (2, 0)      # column 2 has no diagonal


def test_gauss_jordan(model, orc):
    rng = np.random.default_rng(2)
    for n in (1, 2, 63, 64, 65):
        a = rng.standard_normal((n, n)) + n * np.eye(n)
        inv = model.gauss_jordan(a)
        assert np.abs(inv @ a - np.eye(n)).max() < 1e-12
    swap = np.array([[0.0, 2.0, 1.0], [4.0, 1.0, 0.0], [-4.0, 3.0, 5.0]])      # a zero on the diagonal; |4| == |-4|: the smaller row
    assert np.abs(model.gauss_jordan(swap) @ swap - np.eye(3)).max() < 1e-14
    with np.errstate(all="ignore"):
        sing = model.gauss_jordan(np.array([[1.0, 2.0], [2.0, 4.0]]))          # a zero pivot is no error
    assert not np.isfinite(sing).all()
    # the inverse the hierarchy keeps: inv*A_L ~ I
    M = am.AMGModel(model, fdrand_csc(orc, 7, 6, 5))
    L = M.levels[-1]
    assert M.inv is not None and L.n <= 64
    assert np.abs(M.inv @ am.dense_of(L.n, L.A) - np.eye(L.n)).max() < 1e-10


def test_vcycle_is_symmetric_for_a_symmetric_matrix(model, orc):
    csc = fdrand_csc(orc, 9, 8, 7)
    n = len(csc[0]) - 1
    S = sp.csc_matrix((csc[2], csc[1] - 1, csc[0] - 1), shape=(n, n))
    assert abs(S - S.T).max() == 0
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    for kw in ({}, {"presweeps": 2, "postsweeps": 2}, {"max_levels": 2}):
        M = am.AMGModel(model, csc, **kw)
        assert len(M.levels) >= 2
        lhs, rhs = float(np.dot(M.ldiv(a), b)), float(np.dot(a, M.ldiv(b)))
        assert abs(lhs - rhs) <= 1e-12 * (np.linalg.norm(M.ldiv(a)) * np.linalg.norm(b))
    # and it is a contraction that cg can use: far fewer iterations than Jacobi on the same system
    M = am.AMGModel(model, csc)
    ones = np.ones(n)
    it_amg = M.cg(ones, reltol=1e-8)[2]
    it_jac = model.krylov.cg(model.krylov.precon("jacobi", csc, orc), csc, ones, reltol=1e-8)[2]
    assert 2 * it_amg <= it_jac


def scipy_level_sizes(S, max_coarse=64, max_levels=10):
    """a second, independent restatement of the setup with NumPy / SciPy (theta = 0): only the level sizes are compared"""
    sizes = [S.shape[0]]
    S = sp.csr_matrix(S)
    while sizes[-1] > max_coarse and len(sizes) < max_levels:
        n = S.shape[0]
        d = S.diagonal()
        rho = abs(sp.diags(1.0 / d) @ S).sum(axis=1).max()
        G = sp.coo_matrix(abs(S) + abs(S.T))
        e = (G.row != G.col) & (G.data != 0)
        row, col = G.row[e], G.col[e]
        i = np.arange(n, dtype=np.uint64)
        x = (i + np.uint64(1)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(16)
        key = (x << np.uint64(32)) | i
        big = np.uint64(0xFFFFFFFFFFFFFFFF)
        state = np.zeros(n, np.int64)
        while (state == 0).any():
            t = np.where(state == 2, np.uint64(0), np.where(state == 1, big, key))
            t1 = t.copy()
            np.maximum.at(t1, row, t[col])
            t2 = t1.copy()
            np.maximum.at(t2, row, t1[col])
            und = state == 0
            state[und & (t2 == key)] = 1
            state[und & (t2 == big)] = 2
        num = np.cumsum(state == 1) - 1
        nbr = [[] for _ in range(n)]
        for r, c in zip(row, col):
            nbr[r].append(c)
        a1 = np.where(state == 1, num, -1)
        for v in range(n):
            if a1[v] < 0:
                rn = [c for c in sorted(nbr[v]) if state[c] == 1]
                if rn:
                    a1[v] = num[rn[0]]
        agg = a1.copy()
        for v in range(n):
            if agg[v] < 0:
                agg[v] = [a1[c] for c in sorted(nbr[v]) if a1[c] >= 0][0]
        nc = int(num[-1]) + 1
        if nc == n:
            break
        T = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
        P = T - sp.diags(((4.0 / 3.0) / rho) / d) @ S @ T
        S = sp.csr_matrix(P.T @ S @ P)
        sizes.append(nc)
    return sizes


def test_level_sizes_at_16_cubed_against_the_scipy_restatement(model, orc):
    csc = fdrand_csc(orc, 16, 16, 16)
    n = len(csc[0]) - 1
    M = am.AMGModel(model, csc)
    S = sp.csc_matrix((csc[2], csc[1] - 1, csc[0] - 1), shape=(n, n))
    got = [L.n for L in M.levels]
    assert got == scipy_level_sizes(S) and len(got) >= 3 and got[0] == 4096
    assert 1.0 < am.operator_complexity(M.levels) < 2.0


def test_edge_hierarchies(model):
    """n = 0 and n = 1 are valid; max_levels = 1 keeps one level; a diagonal matrix stops where the aggregation stalls"""
    M = am.AMGModel(model, EMPTY)
    assert [L.n for L in M.levels] == [0] and M.ldiv(np.zeros(0)).shape == (0,)
    M = am.AMGModel(model, am.path_graph(1))
    assert [L.n for L in M.levels] == [1] and bits(M.ldiv(np.array([3.0])))[0] == bits(np.array([1.5]))[0]
    M = am.AMGModel(model, am.path_graph(200), max_levels=1)
    assert [L.n for L in M.levels] == [200] and M.inv.shape == (200, 200)
    n = 600
    diag = (np.arange(1, n + 2, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64), 1.0 + np.arange(n) / n)
    M = am.AMGModel(model, diag)
    assert [L.n for L in M.levels] == [n] and M.levels[0].nc == n and M.inv is None      # smoothing only
    v = np.random.default_rng(8).standard_normal(n)
    u = M.ldiv(v)                 # two sweeps of weighted Jacobi on a diagonal matrix: x = w b, then x + w (b - a x)
    w = (4.0 / 3.0) / diag[2]
    np.testing.assert_allclose(u, w * v + w * (v - diag[2] * (w * v)), rtol=1e-14)


def test_entry_points_exist_without_a_gpu(esp):
    hdr = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    names = ["esp_precon_amg_create", "esp_precon_amg_levels", "esp_precon_amg_level", "esp_precon_amg_aggregates",
             "esp_precon_amg_coarse_inverse"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in esp._lib.SIGNATURES
        assert hasattr(esp._lib.load(), name)
    assert re.search(r"#define\s+ESP_PRECON_AMG\s+4\b", hdr) and esp.ESP_PRECON_AMG == 4
    assert re.search(r"#define\s+ESP_AMG_DENSE_MAX\s+512\b", hdr)
    assert esp.SA_AMGPreconditioner is esp.AMGPreconditioner
