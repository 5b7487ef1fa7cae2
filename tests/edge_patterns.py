"""Crafted sparsity patterns (test infrastructure) that put the compile-time capacities of the solve side exactly at their
edges: ILUAM's launch list (a level of 256 / 257 nodes, a fold of exactly 256 / 257 nodes, thin groups between wide launches), the
staging capacity of the row kernels (a 256-row block of 2047 / 2048 / 2049 entries, a single row above the capacity, an empty
part, a ragged last block above it) and, with the tridiagonal matrix, the grid cap of the solvers' vector kernels.

Plain NumPy: the generators return unique 1-based triplets (I, J, V) and n, make no GPU call and import nothing from the
package.  The two helpers at the end take the package as an argument and assemble triplets through append + flush."""
import numpy as np

LT = 256        # iluam.hip: threads of a workgroup = the most nodes the levels of one thin launch hold together
CAP = 2048      # precon.hip PCAP / krylov.hpp KCAP: part entries a workgroup of 256 rows stages in LDS
ROWS = 256      # rows of a workgroup of the row kernels

WIDTHS = {
    "w256": [256],
    "w257": [257],
    "fold_exact": [255, 1, 1],
    "fold_exact2": [1, 255, 1],
    "fold_over": [255, 2, 1],
    "mixed": [128, 128, 1, 256, 257, 1, 1, 512, 3, 513, 1],
    "chain300": [1] * 300,
    "pairs129": [2] * 129,
}
FORMS = ["lower", "upper", "reversed", "symmetric"]
# form -> the schedules (0 factorization columns, 1 forward rows, 2 backward rows) whose level widths are exactly `widths`
PRESCRIBED = {"lower": (1,), "upper": (0,), "reversed": (2,), "symmetric": (0, 1)}


def layered(widths, form, seed=0):
    """Nodes numbered group by group, group l with widths[l] nodes; node t of group l > 0 depends on the nodes t mod w and
    (7t + 3) mod w of group l-1 (w = widths[l-1]).  form: "lower" stores (i, dep) -- the forward rows get `widths` as their
    level widths; "upper" the transpose -- the factorization columns; "reversed" is "lower" with every index i -> n-1-i -- the
    backward rows; "symmetric" both triangles -- forward rows and factorization columns.  Off-diagonal values uniform in
    (-1, 1), every diagonal entry 1 + max(row abs sum, column abs sum).  -> (I, J, V, n), 1-based unique triplets"""
    assert form in FORMS
    widths = [int(w) for w in widths]
    assert all(w > 0 for w in widths)
    n = sum(widths)
    first = np.concatenate([[0], np.cumsum(widths)])
    node, dep = [], []
    for l in range(1, len(widths)):
        w = widths[l - 1]
        t = np.arange(widths[l])
        a, b = t % w, (7 * t + 3) % w
        node.append(first[l] + t)
        dep.append(first[l - 1] + a)
        two = b != a
        node.append(first[l] + t[two])
        dep.append(first[l - 1] + b[two])
    node = np.concatenate(node).astype(np.int64) if node else np.empty(0, np.int64)
    dep = np.concatenate(dep).astype(np.int64) if dep else np.empty(0, np.int64)
    if form == "lower":
        I, J = node, dep
    elif form == "upper":
        I, J = dep, node
    elif form == "reversed":
        I, J = n - 1 - node, n - 1 - dep
    else:
        I, J = np.concatenate([node, dep]), np.concatenate([dep, node])
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1.0, 1.0, len(I))
    V[V == -1.0] = 0.5      # (the interval is open)
    rows = np.bincount(I, weights=np.abs(V), minlength=n)
    cols = np.bincount(J, weights=np.abs(V), minlength=n)
    d = np.arange(n, dtype=np.int64)
    return (np.concatenate([d, I]) + 1, np.concatenate([d, J]) + 1, np.concatenate([1.0 + np.maximum(rows, cols), V]), n)


def widths_of(level):
    """level[node] -> the number of nodes of every level"""
    return [int(c) for c in np.bincount(np.asarray(level, np.int64))]


def launch_list(widths):
    """build_schedule's rule (iluam.hip) restated: a level wider than 256 nodes is a wide launch by itself; else as many
    consecutive levels as together hold at most 256 nodes share one thin launch.  -> (wide launches, thin launches)"""
    wide = thin = 0
    l, nl = 0, len(widths)
    while l < nl:
        if widths[l] > LT:
            wide += 1
            l += 1
            continue
        total = widths[l]
        l += 1
        while l < nl and total + widths[l] <= LT:
            total += widths[l]
            l += 1
        thin += 1
    return wide, thin


# block -> (strictly-lower entries, strictly-upper entries); the diagonal is stored in every row
CAPACITY_N = 9 * ROWS + 37
CAPACITY_BLOCKS = [(2047, 2049), (2048, 2048), (2049, 2047), (895, 896), (896, 896), (896, 897), (1500, 600), (0, 0), (700, 300),
                   (2183, 0)]
CAPACITY_SINGLE_ROW_BLOCK = 6      # all its off-diagonals sit in its first row


def _spread(total, room):
    """`total` entries over rows with room[r] places, as evenly as the room allows: count[r] = min(room[r], L) with the rest one
    each to the first rows that have room left"""
    room = np.asarray(room, np.int64)
    assert 0 <= total <= room.sum()
    lo, hi = 0, int(room.max()) if len(room) else 0
    while lo < hi:                       # the largest L with sum(min(room, L)) <= total
        mid = (lo + hi + 1) // 2
        if np.minimum(room, mid).sum() <= total:
            lo = mid
        else:
            hi = mid - 1
    cnt = np.minimum(room, lo)
    rest = total - int(cnt.sum())
    more = np.flatnonzero(room > lo)[:rest]
    assert len(more) == rest
    cnt[more] += 1
    return cnt


def capacity(seed=0):
    """n = 9*256 + 37 = 2341; the 256-row blocks hold exactly CAPACITY_BLOCKS' strictly-lower and strictly-upper entry counts
    (block 6: all of them in one row, the other rows the diagonal only; block 7: no off-diagonal entry; block 9: 37 rows of 59
    lower entries each), spread as evenly as the room allows (row r has room for r lower and n-1-r upper entries), the columns
    drawn without replacement, off-diagonal values uniform in (-1, 1), the diagonal 1 + row abs sum.
    -> (I, J, V, n), 1-based unique triplets"""
    n = CAPACITY_N
    rng = np.random.default_rng(seed)
    lcnt, ucnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for blk, (nl, nu) in enumerate(CAPACITY_BLOCKS):
        r = np.arange(blk * ROWS, min((blk + 1) * ROWS, n))
        if blk == CAPACITY_SINGLE_ROW_BLOCK:
            assert nl <= r[0] and nu <= n - 1 - r[0]
            lcnt[r[0]], ucnt[r[0]] = nl, nu
        else:
            lcnt[r] = _spread(nl, r)
            ucnt[r] = _spread(nu, n - 1 - r)
    I, J = [], []
    for r in range(n):
        if lcnt[r]:
            J.append(rng.choice(r, lcnt[r], replace=False))
            I.append(np.full(lcnt[r], r, np.int64))
        if ucnt[r]:
            J.append(r + 1 + rng.choice(n - 1 - r, ucnt[r], replace=False))
            I.append(np.full(ucnt[r], r, np.int64))
    I, J = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    V = rng.uniform(-1.0, 1.0, len(I))
    V[V == -1.0] = 0.5
    d = np.arange(n, dtype=np.int64)
    diag = 1.0 + np.bincount(I, weights=np.abs(V), minlength=n)
    return np.concatenate([d, I]) + 1, np.concatenate([d, J]) + 1, np.concatenate([diag, V]), n


def csc_arrays(n, I, J, V):
    """Julia's CSC arrays (1-based colptr and rowval, nzval) of unique 1-based triplets"""
    I, J, V = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(V, np.float64)
    order = np.lexsort((I, J))
    cp = np.ones(n + 1, np.int64)
    np.cumsum(np.bincount(J - 1, minlength=n), out=cp[1:])
    cp[1:] += 1
    return cp, np.ascontiguousarray(I[order]), np.ascontiguousarray(V[order])


def tridiagonal_triplets(n):
    """the non-symmetric tridiagonal (4, -1.5 below, -0.5 above)"""
    d = np.arange(1, n + 1)
    I = np.concatenate([d, d[1:], d[:-1]])
    J = np.concatenate([d, d[:-1], d[1:]])
    V = np.concatenate([np.full(n, 4.0), np.full(max(n - 1, 0), -1.5), np.full(max(n - 1, 0), -0.5)])
    return I, J, V


# ---- the GPU side: `esp` is the package, handed in by the caller --------------------------------------------------------------
def from_triplets(esp, n, I, J, V):
    A = esp.ExtendableSparseMatrix(n, n)
    if len(I):
        A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def tridiagonal(esp, n):
    """the non-symmetric tridiagonal (4, -1.5 below, -0.5 above)"""
    return from_triplets(esp, n, *tridiagonal_triplets(n))
