"""Crafted sparsity patterns (test infrastructure) for the factorization side: the two forms of ILUAM's column factorization
(iluam.hip: a lane per column, FactorOp, and a wave per column, FactorWaveOp) at the switch between them, at the wave form's staging
capacity, lane stride, search outcomes and launch geometry; and graphs for the wave loops of LUFactorization's ordering and fill
(lu.hip: nbr_max with several long vertices in a wave, lu_bfill_k with nodes of 63 / 64 / 65 vertices).

Plain NumPy / SciPy: the generators return unique 1-based triplets (I, J, V, n), make no GPU call and import nothing from the package.
Off-diagonal values are seeded in (-1, 1), every diagonal entry is 1 + max(row abs sum, column abs sum) as in edge_patterns.layered,
so the model's factor is finite.  search_outcomes restates the wave form's bisection on the pattern alone."""
import numpy as np
import scipy.sparse as sp

FW_ROWS = 2048     # iluam.hip FW_ROWS: the rows of column j a wave stages in LDS; a longer column is searched in global memory
FW_MIN_AVG = 24    # iluam.hip FW_MIN_AVG: the automatic rule takes the wave form when nnz >= FW_MIN_AVG * n
WAVE = 64          # the lanes of a wave: the stride of FactorWaveOp over the rows of column i, of nbr_max and of lu_bfill_k
LT = 256           # iluam.hip LT: threads of a workgroup -- LT / WAVE = 4 members per workgroup of the wave form
AMG_LONG = 32      # amg.hpp AMG_LONG (lu.hip's nbr_max): a vertex whose column or row holds more entries is folded by its wave


def _finish(n, I, J, rng):
    """0-based unique off-diagonal positions -> (I, J, V, n): seeded values in (-1, 1), the dominant diagonal in front, 1-based"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    assert np.all(I != J)
    V = rng.uniform(-1.0, 1.0, len(I))
    V[V == -1.0] = 0.5      # (the interval is open)
    return _with_diagonal(n, I, J, V)


def _with_diagonal(n, I, J, V):
    rows = np.bincount(I, weights=np.abs(V), minlength=n)
    cols = np.bincount(J, weights=np.abs(V), minlength=n)
    d = np.arange(n, dtype=np.int64)
    return np.concatenate([d, I]) + 1, np.concatenate([d, J]) + 1, np.concatenate([1.0 + np.maximum(rows, cols), V]), n


def transposed(case):
    """the transpose of a case: rows and columns swapped, the values kept"""
    I, J, V, n = case
    return J, I, V, n


def exact_nnz(n, nnz, seed=0):
    """a full diagonal and nnz - n off-diagonal positions: the first nnz - n of one seeded shuffle of all n (n - 1) of them, with the
    values drawn for the whole shuffle -- exact_nnz(n, k - 1) is exact_nnz(n, k) without its last off-diagonal entry (the diagonals
    follow)"""
    k = nnz - n
    assert 0 <= k <= n * (n - 1)
    rng = np.random.default_rng(seed)
    pos = rng.permutation(n * (n - 1))
    V = rng.uniform(-1.0, 1.0, n * (n - 1))
    V[V == -1.0] = 0.5
    pos, V = pos[:k], V[:k]
    J = pos // (n - 1)
    I = pos % (n - 1)
    I = I + (I >= J)        # (skip the diagonal)
    return _with_diagonal(n, I.astype(np.int64), J.astype(np.int64), V)


def arrowband(n, half=12, hub=None, seed=0):
    """every (i, j) with |i - j| <= half, and a dense column and a dense row at the hub (None: the last index).  The hub's column
    holds n rows.  With the hub last every other column holds the hub's row as its final entry -- every update of the last column lands
    on its position len - 1 -- and the factor schedule is n levels of one column.  hub < n - 1 is the symmetric permutation of that
    matrix which moves the last index to `hub` and keeps the order of the others: the columns behind the hub read the long column as
    their column i."""
    assert n > 2 * half + 2
    i = np.arange(n)
    I, J = [], []
    for d in range(1, half + 1):
        I += [i[d:], i[:-d]]
        J += [i[:-d], i[d:]]
    far = i[:n - 1 - half]          # the rows / columns of the last index outside the band
    I += [far, np.full(len(far), n - 1)]
    J += [np.full(len(far), n - 1), far]
    I, J = np.concatenate(I), np.concatenate(J)
    if hub is not None and hub != n - 1:
        assert 0 <= hub < n - 1
        new = np.where(i < hub, i, i + 1)
        new[n - 1] = hub
        I, J = new[I], new[J]
    return _finish(n, I, J, np.random.default_rng(seed))


def cliques(copies, m, seed=0):
    """block-diagonal: `copies` dense m x m blocks, numbered block by block.  Level l of the factor schedule holds column l of every
    block: m levels of width `copies`; every column holds m entries"""
    b = np.repeat(np.arange(copies), m * m) * m
    r = np.tile(np.repeat(np.arange(m), m), copies)
    c = np.tile(np.tile(np.arange(m), m), copies)
    off = r != c
    return _finish(copies * m, (b + r)[off], (b + c)[off], np.random.default_rng(seed))


def sparse_dense_enough(n=300, density=0.1, seed=3):
    """non-symmetric: the density * n * n seeded positions of scipy.sparse.random and the diagonal -- about density * n entries per
    column, columns that interleave: the wave form's search hits, misses between two rows of column j and runs beyond its last row
    (seed 3: 9270 entries; 9404 hits, 76 903 misses inside, 3719 beyond)"""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density, random_state=rng, format="coo")
    off = S.row != S.col
    return _finish(n, S.row[off], S.col[off], rng)


def search_outcomes(cp, rv):
    """FactorWaveOp's search restated on the pattern (1-based CSC arrays): for every column j, every position v above its diagonal
    (row i) and every row r of column i below ITS diagonal, the first row of column j behind v that is not below r.
    -> (hits, misses inside column j, misses beyond its last row)"""
    n = len(cp) - 1
    cols = [np.asarray(rv[cp[j] - 1:cp[j + 1] - 1]) - 1 for j in range(n)]
    below = [c[c > j] for j, c in enumerate(cols)]
    hit = inside = beyond = 0
    for j, c in enumerate(cols):
        for v in range(int(np.searchsorted(c, j))):
            r = below[c[v]]
            lo = v + 1 + np.searchsorted(c[v + 1:], r)
            found = lo < len(c)
            same = c[np.minimum(lo, len(c) - 1)] == r
            hit += int((found & same).sum())
            inside += int((found & ~same).sum())
            beyond += int((~found).sum())
    return hit, inside, beyond


# ---- graphs for LUFactorization ------------------------------------------------------------------------------------------------------
def multi_hub(n, hubs, entries, by, seed=0):
    """the path 0 - 1 - ... - n-1 (stored both ways, it keeps the graph connected) and, for every listed hub, `entries` seeded
    neighbours among the vertices that are neither hubs nor the hub's path neighbours, stored in the hub's column (by = "col": the
    entries (v, hub)), in its row ("row": (hub, v)) or both ("both")"""
    assert by in ("col", "row", "both")
    rng = np.random.default_rng(seed)
    i = np.arange(n - 1)
    I, J = [i + 1, i], [i, i + 1]
    for h in hubs:
        ok = np.array([v for v in range(n) if v not in hubs and abs(v - h) > 1])
        nb = np.sort(rng.choice(ok, entries, replace=False))
        if by in ("col", "both"):
            I.append(nb)
            J.append(np.full(entries, h))
        if by in ("row", "both"):
            I.append(np.full(entries, h))
            J.append(nb)
    return _finish(n, np.concatenate(I), np.concatenate(J), rng)


MULTI_HUB_N = 300      # five waves: the last one, the first of the second workgroup, has 44 live lanes
HUB_SETS = [[0], [63], [0, 63], [10, 11], [64, 100, 127], [299]]
# every hub set long by its column alone at 33 neighbours and by its row alone at 65; lanes 0 and 63 together also by both
MULTI_HUB_CASES = [(hubs, e, by) for hubs in HUB_SETS for e, by in ((33, "col"), (65, "row"))] + [([0, 63], 33, "both"), ([0, 63], 65, "both")]


def long_vertices(cp, rv):
    """nbr_max's rule on the pattern (1-based CSC arrays): the vertices whose column / whose row holds more than AMG_LONG entries
    -> (long by column, long by row), ascending 0-based indices"""
    n = len(cp) - 1
    percol = np.diff(cp)
    perrow = np.bincount(np.asarray(rv) - 1, minlength=n)
    return np.flatnonzero(percol > AMG_LONG), np.flatnonzero(perrow > AMG_LONG)


def clique_components(sizes, tail=0, seed=0):
    """cliques of the given sizes as separate components, numbered one after the other; tail > 0: every clique's last vertex is joined
    by one edge to a path of `tail` further vertices that follow it.  Both triangles are stored."""
    I, J, base = [], [], 0
    for m in sizes:
        r, c = np.nonzero(~np.eye(m, dtype=bool))
        I.append(base + r)
        J.append(base + c)
        base += m
        if tail:
            a = np.arange(base - 1, base + tail - 1)     # the clique's last vertex, then the path
            I += [a + 1, a]
            J += [a, a + 1]
            base += tail
    return _finish(base, np.concatenate(I), np.concatenate(J), np.random.default_rng(seed))


# (sizes, tail) whose clique-side leaves hold exactly 63, 64, 65 vertices under leaf_size 70 (tests/test_edge_patterns.py shows it)
CLIQUE_TAILS_AT_THE_EDGE = ([59, 60, 61], 12)
