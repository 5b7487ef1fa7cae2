"""Crafted sparsity patterns (test infrastructure) for the approximate-inverse and threshold side: SPAIPreconditioner's two tiers,
the two forms of its size pass and SPAI-0 (spai.hip) at the edges of their capacities, and the look-up branch of ILUTPreconditioner's
sweep (ilut.hip: a short row against a long column) with every one of its ends.

Plain NumPy / SciPy: the generators return host CSC arrays in Julia's convention (colptr, rowval 1-based, nzval), make no GPU call
and import nothing from the package.  Values are seeded.  Where a SPAI column is meant for a comparison with lstsq its local problem
is well conditioned: the diagonal is 4 + U(0,1) and the off-diagonals of a column of len rows are U(-1,1) / (2 len), so every column
that stores its diagonal is strictly diagonally dominant; a column without a diagonal has entries below 1/2 in sum.
column_sizes, spai_tier and sweep_outcomes restate the device's rules on the arrays alone."""
import numpy as np

from spai_modellib import csc_from_columns, hub_columns, sized_columns

SORT_MAX = 16384     # spai.hip SORT_MAX: the rows the workgroup form of the size pass sorts; more are refused with a bound of p
SIZE_WAVE = 512      # spai.hip: the wave form of the size pass takes the lists of at most ESP_SPAI_WAVE_DOUBLES rows together
GRID_MAX = 1 << 20   # spai.hip GRID_MAX: workgroups of the grid-stride launches of the wave tier
RGRID = 1024         # spai.hip: workgroups (and R slots) of the workgroup tier's launch, at most; see r_slots
R_DOUBLES = 1 << 27  # spai.hip: the doubles (1 GiB) that the R slots of one launch may take together
WAVE = 64            # lanes of a wave: the stride of the ordered sum and of spai0_k
TIER_WAVE, TIER_WIDE, TIER_REFUSED, TIER_REFUSED_BOUND = "wave", "wide", "refused", "refused_bound"


# ---- values ------------------------------------------------------------------------------------------------------------------------
def dominant_csc(cols, rng):
    """Julia CSC arrays of the pattern cols (cols[j] = the stored rows of column j, 0-based): 4 + U(0,1) on the diagonal, U(-1,1)
    divided by twice the column's length elsewhere"""
    lens = np.array([len(c) for c in cols], np.int64)
    cp = np.ones(len(cols) + 1, np.int64)
    np.cumsum(lens, out=cp[1:])
    cp[1:] += 1
    rows = np.concatenate([np.sort(np.asarray(c, np.int64)) for c in cols] + [np.zeros(0, np.int64)])
    colof = np.repeat(np.arange(len(cols), dtype=np.int64), lens)
    for j, c in enumerate(cols):
        assert len(set(int(r) for r in c)) == len(c), j
    off = rng.uniform(-1.0, 1.0, len(rows)) / (2.0 * np.maximum(lens[colof], 1))
    nz = np.where(rows == colof, 4.0 + rng.random(len(rows)), off)
    return cp, rows + 1, nz


# ---- SPAI-1 ------------------------------------------------------------------------------------------------------------------------
def dense_block(m, seed=0):
    """n = m, every column stores every row: p = q = m and the lists hold tc = m*m rows together, every row m times"""
    return dominant_csc([list(range(m)) for _ in range(m)], np.random.default_rng(1000 + m + seed))


def full_lists_columns(p, q):
    """n = p > q.  Column 0 stores the rows 1..q (no diagonal); the columns 1..q store the rows 0..p-1, all of them the same; the
    columns beyond store their diagonal alone.  Column 0 has q unknowns over p rows and tc = p*q exactly: every list is full."""
    assert p > q >= 1
    return [list(range(1, q + 1))] + [list(range(p)) for _ in range(q)] + [[j] for j in range(q + 1, p)]


def full_lists(p, q, seed=0):
    return dominant_csc(full_lists_columns(p, q), np.random.default_rng(2000 + p + seed))


def fan_columns(p, q, shared=False):
    """n = p + q.  Column 0 stores the rows 1..q (no diagonal); the columns 1..q deal the p rows 0, q+1, .., p+q-1 among them in
    contiguous shares (column 1 holds row 0); every other column is empty.  Column 0 has q unknowns over p rows with p / q as large
    as one likes: a column c of 1..q has p / q unknowns of its own, but the columns of its unknowns are empty (or column 0), so its
    own problem has at most q rows -- a column that stored its diagonal would have a problem of (p / q)^2 doubles at least, which
    ESP_SPAI_DENSE_MAX refuses beyond p / q = 110.  The shares do not meet: column 0's B has orthogonal columns.
    shared: every one of the columns 1..q stores all p rows instead, so column 0 has tc = p q, every row q times, and each of those
    columns has p unknowns over the q rows of column 0."""
    assert p >= q >= 1
    rows = [0] + list(range(q + 1, p + q))
    cols = [list(range(1, q + 1))]
    for c in range(q):
        cols.append(list(rows) if shared else rows[c * p // q:(c + 1) * p // q])
    return cols + [[] for _ in range(q + 1, p + q)]


def fan(p, q, shared=False, seed=0):
    return dominant_csc(fan_columns(p, q, shared), np.random.default_rng(3000 + p + seed))


def sized(p, q, seed=0):
    """spai_modellib.sized_columns with the dominant values: column 0 has q unknowns, p rows and tc = p + q - 1"""
    return dominant_csc(sized_columns(p, q), np.random.default_rng(4000 + p + seed))


def hub(h, seed=0):
    """spai_modellib.hub_columns with its own values: the hub (column 0) has q = h unknowns over 3 rows, rank-deficient"""
    return csc_from_columns(hub_columns(h), np.random.default_rng(5000 + h + seed))


def block_diagonal(blocks):
    """the block diagonal matrix of column lists"""
    cols, at = [], 0
    for b in blocks:
        cols += [[r + at for r in c] for c in b]
        at += len(b)
    return cols


def many_wide_columns(count, qa=23, qb=40):
    """`count` hub blocks, hub_columns(qa) and hub_columns(qb) in turn: one workgroup-tier column per block, q = qa and qb"""
    return block_diagonal([hub_columns(qa if t % 2 == 0 else qb) for t in range(count)])


def many_wide(count, qa=23, qb=40, seed=0):
    return csc_from_columns(many_wide_columns(count, qa, qb), np.random.default_rng(6000 + count + seed))


def tridiagonal(n, seed=0):
    """the tridiagonal matrix of order n: every column in the wave tier (p <= 5, q <= 3)"""
    rng = np.random.default_rng(7000 + seed)
    j = np.arange(n, dtype=np.int64)
    lens = np.full(n, 3, np.int64)
    lens[0] = lens[-1] = 2 if n > 1 else 1
    cp = np.ones(n + 1, np.int64)
    np.cumsum(lens, out=cp[1:])
    cp[1:] += 1
    colof = np.repeat(j, lens)
    k = np.arange(len(colof), dtype=np.int64) - (cp[colof] - 1)
    rows = colof - 1 + k + (colof == 0)
    nz = np.where(rows == colof, 4.0 + rng.random(len(rows)), rng.uniform(-1.0, 1.0, len(rows)) / 6.0)
    return cp, rows + 1, nz


def column_sizes(csc, k):
    """(p, q, tc, maxlen) of column k from the arrays alone: q its stored rows, tc the rows of their columns' lists together, p the
    size of the union, maxlen the longest list"""
    cp, rv = csc[0], csc[1]
    J = rv[cp[k] - 1:cp[k + 1] - 1] - 1
    lists = [rv[cp[j] - 1:cp[j + 1] - 1] for j in J]
    tc = int(sum(len(l) for l in lists))
    p = len(np.unique(np.concatenate(lists))) if tc else 0
    return p, len(J), tc, max([len(l) for l in lists], default=0)


def all_sizes(csc):
    """(p, q, tc) of every column as arrays (vectorised over the lists: for the matrices of 10^4 columns and more)"""
    import scipy.sparse as sp
    cp, rv = csc[0], csc[1]
    n = len(cp) - 1
    P = sp.csc_matrix((np.ones(len(rv)), rv - 1, cp - 1), shape=(n, n))
    lens = np.diff(cp).astype(np.int64)
    q = lens.copy()
    tc = np.asarray(P.T @ lens).ravel().astype(np.int64)        # sum over the stored rows j of column k of len(column j)
    U = (P @ P).tocsc()                                          # pattern: row r is in some column j that column k stores
    p = np.diff(U.indptr).astype(np.int64)
    return p, q, tc


def spai_tier(p, q, tc, maxlen, wave_doubles, dense_max):
    """spai_size_k's rule -> (tier, the p it reports)"""
    if q == 0:
        return TIER_WAVE, 0
    if tc > SORT_MAX:
        return TIER_REFUSED_BOUND, max(maxlen, -(-tc // q))
    if p * q > dense_max:
        return TIER_REFUSED, p
    if p * q <= wave_doubles and q * q <= wave_doubles:
        return TIER_WAVE, p
    return TIER_WIDE, p


def r_slots(nwide, wideq):
    """the workgroups of the workgroup tier's launch, one R slot of wideq^2 doubles each: as many as there are listed columns, at most
    RGRID, and at most what R_DOUBLES holds (at least one)"""
    return max(1, min(nwide, RGRID, R_DOUBLES // max(wideq * wideq, 1)))


def size_form(tc):
    """which form of the size pass counts a column's rows: the wave form up to SIZE_WAVE rows, the workgroup form beyond"""
    return "wave" if tc <= SIZE_WAVE else "group"


# ---- SPAI-0 ------------------------------------------------------------------------------------------------------------------------
SPAI0_N = 211
# column: (first row, last row, left out) -- the stored rows are first..last without `left out`
SPAI0_COLUMNS = {
    5: (0, 62, None),        # 63 rows, the diagonal at position 5: the first lane stride
    70: (7, 70, None),       # 64 rows, the diagonal at position 63: the last lane of the first stride
    100: (36, 100, None),    # 65 rows, the diagonal at position 64: the second stride, lane 0
    150: (21, 150, None),    # 130 rows, the diagonal the last entry (position 129): the third stride, lane 1
    160: (0, 199, None),     # 200 rows, the diagonal at position 160: the third stride of four
    180: (0, 200, 180),      # 200 rows, no diagonal
    190: (81, 210, None),    # 130 rows, the diagonal at position 109: the second stride
    200: None,               # empty
}


def spai0_columns():
    cols = [[j] for j in range(SPAI0_N)]
    for j, spec in SPAI0_COLUMNS.items():
        cols[j] = [] if spec is None else [r for r in range(spec[0], spec[1] + 1) if r != spec[2]]
    return cols


def spai0_matrix(special=False, seed=0):
    """n = 211 (three live waves in the last workgroup of four).  special: a NaN at position 170 of column 160 (third stride) and an
    Inf at position 10 of column 150"""
    cp, rv, nz = csc_from_columns(spai0_columns(), np.random.default_rng(8000 + seed))
    if special:
        nz[cp[160] - 1 + 170] = np.nan
        nz[cp[150] - 1 + 10] = np.inf
    return cp, rv, nz


def diagonal_position(csc, j):
    """the position of row j among column j's stored rows, or -1"""
    cp, rv = csc[0], csc[1]
    rows = rv[cp[j] - 1:cp[j + 1] - 1] - 1
    at = np.flatnonzero(rows == j)
    return int(at[0]) if len(at) else -1


# ---- ILUT --------------------------------------------------------------------------------------------------------------------------
COMB_GAP = 48       # columns between the last upper row of the long column and the long column
COMB_BELOW = 48     # rows below the long column's diagonal


def comb(up, L, seed=0):
    """One long column j with `up` rows K above its diagonal, every other row from 2 L + 1 on (K = 2L+1, 2L+3, ..), a stretch of
    COMB_GAP columns between max K and j, and COMB_BELOW rows below the diagonal; n = j + 1 + COMB_BELOW.  Every column but j stores
    the row above its diagonal, so the merge branch has products to subtract.  Every row i that column j stores (K and i > j) holds
    exactly L entries: its diagonal, (i, i+1), (i, j) and columns left of min(i, j) -- pairs (k, k+1) with k in K, a hit and a miss
    between two members of K, and, for two of every three rows i > j, two columns of the gap: beyond max K, where the look-up
    ends with c == up.  The other rows i > j and the rows of K end at a column >= min(i, j).  8 L < up: all of them take the look-up
    branch in column j; every other column has one row above its diagonal, and the merge runs.  Off-diagonals have magnitudes in
    [0.25, 1), every diagonal is 1 + max(row abs sum, column abs sum).
    -> ((colptr, rowval, nzval), j)"""
    assert L >= 5
    rng = np.random.default_rng(9000 + 7 * up + L + seed)
    base = 2 * L
    K = base + 1 + 2 * np.arange(up, dtype=np.int64)
    j = int(K[-1]) + 1 + COMB_GAP
    n = j + 1 + COMB_BELOW
    I, J = [np.arange(n)], [np.arange(n)]
    sup = np.array([c for c in range(1, n) if c != j], np.int64)      # (c - 1, c)
    I.append(sup - 1)
    J.append(sup)
    below = np.arange(j + 1, n, dtype=np.int64)
    I += [K, below]
    J += [np.full(up, j), np.full(len(below), j)]

    def left_columns(count, members, gaps):
        """`count` ascending columns: `gaps` of the gap stretch, the others pairs (k, k+1) of `members` (a single k when odd)"""
        take = count - gaps
        ks = np.sort(rng.choice(members, size=(take + 1) // 2, replace=False))
        out = np.concatenate([ks, ks[:take // 2] + 1])
        g = np.sort(rng.choice(np.arange(K[-1] + 1, j), size=gaps, replace=False)) if gaps else np.zeros(0, np.int64)
        return np.sort(np.concatenate([out, g]))
    for i in K:                                                       # L - 3 columns left of i
        if i == K[0]:
            cols = np.arange(L - 3, dtype=np.int64) * 2               # below base: misses in front of K's first member
        else:
            members = K[K < i]
            if len(members) >= (L - 2) // 2:
                cols = left_columns(L - 3, members, 0)
            else:
                cols = np.sort(rng.choice(np.arange(0, i), size=L - 3, replace=False))
        assert len(np.unique(cols)) == L - 3 and cols.max() < i
        I.append(np.full(L - 3, i))
        J.append(cols)
    for t, i in enumerate(below):
        count = L - 3 if i < n - 1 else L - 2                         # (the last row has no (i, i+1))
        gaps = 0 if t % 3 == 2 else (2 if count >= 4 else 1)
        cols = left_columns(count, K[:-1], gaps)
        assert len(np.unique(cols)) == count
        I.append(np.full(count, i))
        J.append(cols)
    I, J = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    assert len(np.unique(I * n + J)) == len(I)
    off = I != J
    V = rng.uniform(0.25, 1.0, len(I)) * rng.choice([-1.0, 1.0], len(I))
    rowsum = np.bincount(I[off], weights=np.abs(V[off]), minlength=n)
    colsum = np.bincount(J[off], weights=np.abs(V[off]), minlength=n)
    V[~off] = 1.0 + np.maximum(rowsum, colsum)[I[~off]]
    order = np.lexsort((I, J))
    cp = np.ones(n + 1, np.int64)
    np.cumsum(np.bincount(J, minlength=n), out=cp[1:])
    cp[1:] += 1
    return (cp, I[order] + 1, V[order]), j


def switch_pair(L, seed=0):
    """the twins on either side of the sweep's switch: comb(8 L, L) -- (re - ra) * 8 < up is false, the merge -- and comb(8 L + 1, L),
    the look-up; the rows that the long column stores hold exactly L entries"""
    return comb(8 * L, L, seed), comb(8 * L + 1, L, seed)


def upper_counts(csc):
    """the rows above the diagonal of every column"""
    cp, rv = csc[0], csc[1]
    n = len(cp) - 1
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    return np.bincount(cols[rv < cols] - 1, minlength=n)


def sweep_outcomes(csc):
    """ilut_sweep_k's choice and the ends of its look-up restated on the pattern alone, a searchsorted per key.
    -> {"merge": entries that take the merge, "lookup": entries that take the look-up, "hit", "miss", "exhausted" (c == up),
    "bound" (ka >= m): keys of the look-up by their end, "carried": keys searched from a lower bound c > 0}"""
    import scipy.sparse as sp
    cp, rv = csc[0], csc[1]
    n = len(cp) - 1
    R = sp.csc_matrix((np.ones(len(rv)), rv - 1, cp - 1), shape=(n, n)).tocsr()
    R.sort_indices()
    rp, rc = R.indptr, R.indices
    ups = upper_counts(csc)
    out = dict(merge=0, lookup=0, hit=0, miss=0, exhausted=0, bound=0, carried=0)
    for j in range(n):
        up = int(ups[j])
        rows = rv[cp[j] - 1:cp[j + 1] - 1] - 1
        lens = rp[rows + 1] - rp[rows]
        look = lens * 8 < up
        out["merge"] += int((~look).sum())
        out["lookup"] += int(look.sum())
        if not look.any():
            continue
        upper = rows[:up]
        for i in rows[look]:
            m = min(int(i), j)
            c = 0
            for ka in rc[rp[i]:rp[i + 1]]:
                if ka >= m:
                    out["bound"] += 1
                    break
                if c > 0:
                    out["carried"] += 1
                c += int(np.searchsorted(upper[c:], ka))
                if c == up:
                    out["exhausted"] += 1
                    break
                if upper[c] != ka:
                    out["miss"] += 1
                    continue
                out["hit"] += 1
                c += 1
    return out
