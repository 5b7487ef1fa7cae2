"""Crafted patterns (test infrastructure) that put the compile-time capacities of the algebra and set-up side exactly at their
edges: the shared column sorts (linalg.hip / internal.hpp), the wave compaction of block.hip, the 2048-entry tiles of the
entry-parallel kernels, the 1024-element tiles of the A+-B merge path, the whole-wave columns of transpose(A)*x and of the AMG
restriction, the reduction grids of norm and opnorm, and the lane / workgroup expansion of ILU(k)'s search.

Plain NumPy: every builder returns host CSC arrays (colptr and rowval 1-based, rows ascending in every column, nzval), makes no GPU
call and imports nothing from the package.  tests/test_edge_patterns.py asserts, from the arrays alone, what is claimed here."""
import numpy as np

COLSORT_LANE = 32       # internal.hpp: a column of at most this many entries is sorted by one lane (templates of 8, 16, 32)
COLSORT_BLOCK = 4096    # ... at most this many by one workgroup in LDS; above: the generic route
BK_LONG = 32            # block.hip: a column with more stored entries is compacted by its whole wave
TILE = 2048             # linalg.hip TP_TILE = matops.hip DS_TILE: entries per workgroup of the entry-parallel kernels
MM_TILE = 1024          # matops.hip: merged elements per tile of A+-B
MV_LONG = 64            # linalg.hip: transpose(A)*x folds a longer column with the whole wave (amg.hip AMG_TLONG is the same)
AMG_LONG = 32           # amg.hip: a longer column of the strength / aggregation kernels is taken by the whole wave
RED_MT = 256            # linalg.hip MT: values per workgroup and round of the norm's reductions
RED_GRID = 1024         # linalg.hip: workgroups of a norm reduction at most -> a second round from 262 145 values on
MAX_GRID = 2048         # linalg.hip: workgroups of segsum_max_k / tp_lens_k at most -> a second round from 524 289 segments on
SHORT_COL = 16          # iluk.hip: a frontier vertex with more stored rows is expanded by the whole workgroup

NAN_PAYLOAD = np.array([0x7FF800000000BEEF], np.uint64).view(np.float64)[0]
NEG_ZERO = np.float64(-0.0)


def csc_from_coo(n_cols, I, J, V):
    """CSC arrays (1-based) of distinct 0-based positions (I, J)"""
    I, J, V = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(V, np.float64)
    order = np.lexsort((I, J))
    cp = np.ones(n_cols + 1, np.int64)
    np.cumsum(np.bincount(J, minlength=n_cols), out=cp[1:])
    cp[1:] += 1
    return cp, np.ascontiguousarray(I[order] + 1), np.ascontiguousarray(V[order])


def transpose_csc(m, csc):
    """the transpose of an m x n CSC as CSC arrays (a stable counting sort by row: plain NumPy, values moved as they are)"""
    cp, rv, nz = csc
    n = len(cp) - 1
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    order = np.argsort(rv, kind="stable")
    cpT = np.ones(m + 1, np.int64)
    np.cumsum(np.bincount(rv - 1, minlength=m), out=cpT[1:])
    cpT[1:] += 1
    return cpT, np.ascontiguousarray(cols[order] + 1), np.ascontiguousarray(nz[order])


# ---- the column sorts -----------------------------------------------------------------------------------------------------------
SORT_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096]
SORT_MAXIMA = [8, 9, 16, 17, 32, 33, 4096, 4097]      # the lane templates change at 8|9 and 16|17, the lane sort ends at 32|33,
SORT_ROWS = 5000                                      # the workgroup sort at 4096|4097 (4097 is appended to SORT_LENGTHS for it)


def sort_sublists():
    """maximum -> the lengths of SORT_LENGTHS (+ [4097]) up to it: the maximum decides which template is launched"""
    return {mx: [l for l in SORT_LENGTHS + [4097] if l <= mx] for mx in SORT_MAXIMA}


def _special_values(nz, where):
    """a stored 0.0, a -0.0 and a NaN with a payload at the three positions `where`"""
    for p, s in zip(where, (0.0, NEG_ZERO, NAN_PAYLOAD)):
        nz[p] = s


def prescribed_lengths(lengths, n_rows=SORT_ROWS, seed=0):
    """n_rows x len(lengths): column j stores exactly lengths[j] distinct rows drawn over the whole row range (the entries of a
    column lie far apart: its transpose scatters them from many tiles).  Values standard normal; the longest column holds a
    stored 0.0 as its first entry, a -0.0 in its middle and a NaN with a payload as its last."""
    rng = np.random.default_rng(seed)
    lengths = [int(l) for l in lengths]
    assert max(lengths) <= n_rows
    rows = [np.sort(rng.choice(n_rows, L, replace=False)) + 1 for L in lengths]
    cp = np.concatenate([[1], 1 + np.cumsum(lengths)]).astype(np.int64)
    rv = np.concatenate(rows).astype(np.int64) if sum(lengths) else np.zeros(0, np.int64)
    nz = rng.standard_normal(len(rv))
    j = int(np.argmax(lengths))
    s, L = cp[j] - 1, lengths[j]
    if L >= 3:
        _special_values(nz, (s, s + L // 2, s + L - 1))
    return cp, rv, nz


def prescribed_square(lengths, seed=0):
    """square, a full diagonal: the t-th listed column (lengths[t] >= 1, its diagonal entry counted) sits at column
    (t * n) // len(lengths) and stores exactly lengths[t] rows; every other column stores its diagonal entry only.
    n = max(96, max(lengths) + 3).  Diagonal 4 + U(0, 1), off-diagonal 1e-3 * normal with a stored 0.0 and a -0.0 in the longest
    column (no NaN: the inner factorizations stay finite).  -> (colptr, rowval, nzval), n, the listed columns (0-based)"""
    lengths = [int(l) for l in lengths]
    assert min(lengths) >= 1
    n = max(96, max(lengths) + 3)
    rng = np.random.default_rng(seed)
    where = [(t * n) // len(lengths) for t in range(len(lengths))]
    assert len(set(where)) == len(where)
    I, J, V = [np.arange(n)], [np.arange(n)], [4.0 + rng.random(n)]
    for c, L in zip(where, lengths):
        others = np.delete(np.arange(n), c)
        r = rng.choice(others, L - 1, replace=False)
        I.append(r)
        J.append(np.full(L - 1, c))
        V.append(1e-3 * rng.standard_normal(L - 1))
    cp, rv, nz = csc_from_coo(n, np.concatenate(I), np.concatenate(J), np.concatenate(V))
    c = where[int(np.argmax(lengths))]
    off = [k for k in range(cp[c] - 1, cp[c + 1] - 1) if rv[k] - 1 != c]
    if len(off) >= 2:
        nz[off[0]], nz[off[-1]] = 0.0, NEG_ZERO
    return (cp, rv, nz), n, where


def worst_case_partitions(n, seed=5):
    """name -> one partitioning (0-based) of 0..n-1: every column reaches the sorts strictly descending (`reversed`), in a seeded
    random order (`shuffled`), and as a descending run followed by an ascending one (`zigzag`: two partitions)"""
    ev, od = np.arange(0, n, 2), np.arange(1, n, 2)
    return {"reversed": [np.arange(n - 1, -1, -1)], "shuffled": [np.random.default_rng(seed).permutation(n)],
            "zigzag": [ev[::-1].copy(), od]}


# ---- BK_LONG ----------------------------------------------------------------------------------------------------------------------
BK_CASES = [(32, 0), (32, 1), (32, 16), (32, 31), (32, 32), (33, 0), (33, 1), (33, 16), (33, 31), (33, 32), (33, 33)]


def compaction_edges(seed=3):
    """n = 200, the partitions [even indices, odd indices]: case t = (stored, kept) of BK_CASES is column t (even and odd columns
    alike), which stores exactly `stored` entries and keeps exactly `kept` of them -- rows of its own parity, interleaved with the
    dropped rows of the other parity; a stored 0.0, a -0.0 and a NaN with a payload among the kept values of the (33, 33) column.
    Every other column stores its diagonal entry.  -> (colptr, rowval, nzval), n, [even, odd]"""
    n = 200
    rng = np.random.default_rng(seed)
    I, J = [], []
    for t, (stored, kept) in enumerate(BK_CASES):
        mine = np.arange(t % 2, n, 2)
        other = np.arange(1 - t % 2, n, 2)
        r = np.concatenate([mine[:kept], other[:stored - kept]])      # both ascending from the top: interleaved after the sort
        I.append(r)
        J.append(np.full(stored, t))
    for j in range(len(BK_CASES), n):
        I.append([j])
        J.append([j])
    I, J = np.concatenate(I), np.concatenate(J)
    cp, rv, nz = csc_from_coo(n, I, J, 1.0 + rng.random(len(I)))
    t = BK_CASES.index((33, 33))
    s = cp[t] - 1
    _special_values(nz, (s + 1, s + 16, s + 32))
    return (cp, rv, nz), n, [np.arange(0, n, 2), np.arange(1, n, 2)]


# ---- tile borders -----------------------------------------------------------------------------------------------------------------
BORDERED_ROWS = 5000
BORDERED_LENGTHS = ([0, 0, 2048, 0, 0, 0, 1000, 500, 4095, 300, 250]
                    + [0, 1, 64, 0, 0, 65, 200, 33, 1, 0, 500, 17, 300, 0, 2, 400, 0, 100, 31, 0, 150, 32, 99, 52, 1]
                    + [0, 0, 0, 0])


def bordered(seed=1):
    """5000 x 40, nnz = 5 * 2048 + 1.  Two leading empty columns; column 2 is exactly the first tile; the border 2048 is the start of
    column 6 behind three empty columns; 4096 and 6144 lie inside column 8 (4095 entries); 8192 is the last entry of column 10;
    10240, the single entry of the last tile, is column 35 alone; four trailing empty columns.  Values as prescribed_lengths."""
    assert len(BORDERED_LENGTHS) == 40 and sum(BORDERED_LENGTHS) == 5 * TILE + 1
    return prescribed_lengths(BORDERED_LENGTHS, BORDERED_ROWS, seed)


def column_of(cp, p):
    """the 0-based column of the 0-based storage position p"""
    return int(np.searchsorted(cp - 1, p, side="right") - 1)


SYM_N = 3000
SYM_POSITIONS = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]      # and nnz - 1: the first and last entry of every tile touched


def symmetric_bordered():
    """square, n = 3000, nnz = 3 * 2048 + 1: the diagonal except (0, 0) and (n-1, n-1), 1571 off-diagonal pairs with equal values
    and five stored zeros (0.0 and -0.0) that have no mirror.  The seed is the first for which the storage positions of
    SYM_POSITIONS and nnz - 1 are off-diagonal, non-zero entries.  -> (colptr, rowval, nzval)"""
    n = SYM_N
    for seed in range(400):
        rng = np.random.default_rng(seed)
        cells = set()
        pairs = [(1500, 0), (n - 1, 1400)]
        cells.update(pairs)
        while len(pairs) < 1571:
            i, j = int(rng.integers(1, n)), int(rng.integers(0, n))
            if i > j and (i, j) not in cells:
                cells.add((i, j))
                pairs.append((i, j))
        zeros = []
        while len(zeros) < 5:
            i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
            if i != j and (max(i, j), min(i, j)) not in cells and (i, j) not in zeros and (j, i) not in zeros:
                zeros.append((i, j))
        pv = rng.standard_normal(len(pairs))
        d = np.arange(1, n - 1)
        I = np.concatenate([d, [p[0] for p in pairs], [p[1] for p in pairs], [z[0] for z in zeros]])
        J = np.concatenate([d, [p[1] for p in pairs], [p[0] for p in pairs], [z[1] for z in zeros]])
        V = np.concatenate([4.0 + rng.random(n - 2), pv, pv, [0.0, NEG_ZERO, 0.0, NEG_ZERO, 0.0]])
        cp, rv, nz = csc_from_coo(n, I, J, V)
        assert len(rv) == 3 * TILE + 1
        ok = True
        for p in SYM_POSITIONS + [len(rv) - 1]:
            ok = ok and rv[p] - 1 != column_of(cp, p) and nz[p] != 0.0
        if ok:
            return cp, rv, nz
    raise AssertionError("no seed puts off-diagonal entries at the tile borders")


def mirror_position(csc, p):
    """the storage position of the mirror (j, i) of the entry (i, j) at position p, or -1"""
    cp, rv, _ = csc
    j = column_of(cp, p)
    i = int(rv[p] - 1)
    s, e = cp[i] - 1, cp[i + 1] - 1
    k = s + int(np.searchsorted(rv[s:e], j + 1))
    return int(k) if k < e and rv[k] == j + 1 else -1


def perturbed(csc, p):
    """a copy with exactly the value at storage position p changed (+ 1.0)"""
    cp, rv, nz = csc
    nz = nz.copy()
    nz[p] += 1.0
    return cp, rv, nz


def zero_pair(csc, p):
    """a copy with the entry at position p a stored 0.0 and its mirror a stored -0.0"""
    cp, rv, nz = csc
    nz = nz.copy()
    q = mirror_position(csc, p)
    assert q >= 0 and q != p
    nz[p], nz[q] = 0.0, NEG_ZERO
    return cp, rv, nz


# ---- the A+-B merge path ----------------------------------------------------------------------------------------------------------
def merged_stream(A, B):
    """the merge path restated: A's and B's entries as (column, row, source) sorted by (column, row), A first on equal keys.
    -> list of (col0, row1, src, position in its operand's storage)"""
    out = []
    for src, (cp, rv, _) in enumerate((A, B)):
        cols = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
        out.extend((int(c), int(r), src, k) for k, (c, r) in enumerate(zip(cols, rv)))
    out.sort(key=lambda t: (t[0], t[1], t[2]))
    return out


def kept_per_tile(A, B, sub):
    """stored results per tile of MM_TILE merged elements (an entry belongs to the tile of its A half, or of its B element when
    no A element shares its key): v = a +- b, a +- 0.0 or 0.0 +- b, kept unless v == 0"""
    st = merged_stream(A, B)
    ntiles = (len(st) + MM_TILE - 1) // MM_TILE
    kept = [0] * ntiles
    for q, (c, r, src, k) in enumerate(st):
        if src == 0:
            pair = q + 1 < len(st) and st[q + 1][:3] == (c, r, 1)
            b = B[2][st[q + 1][3]] if pair else 0.0
            v = A[2][k] - b if sub else A[2][k] + b
        else:
            if q > 0 and st[q - 1][:3] == (c, r, 0):
                continue
            v = 0.0 - B[2][k] if sub else 0.0 + B[2][k]
        if not v == 0.0:
            kept[q // MM_TILE] += 1
    return kept


def _one_column(m, rows_a, vals_a, rows_b, vals_b):
    z = np.zeros
    return (csc_from_coo(1, np.asarray(rows_a) - 1, z(len(rows_a), np.int64), vals_a),
            csc_from_coo(1, np.asarray(rows_b) - 1, z(len(rows_b), np.int64), vals_b), m)


def _random_cells(rng, m, n, k):
    flat = rng.choice(m * n, k, replace=False)
    return flat % m, flat // m


def merge_cases(seed=11):
    """name -> dict(A, B, m, total = nnz(A) + nnz(B), and what the case claims; tests/test_edge_patterns.py checks every claim
    with merged_stream / kept_per_tile):
      split          one column, A row 1 alone, then the rows 2..1100 in both: the pair of row 513 is the merged elements 1023 | 1024,
                     the pair of row 1025 the elements 2047 | 2048 (`split_pairs`: (A position, B position) in the merged order)
      split_cancel   the same pattern; b = -a at row 513 (cancels under +), b = a at row 1025 (cancels under -)
      a_exhausted    A: 100 entries at the top of column 0; B: 3100 entries in three columns -> the tiles 1, 2, 3 hold B elements only
      b_exhausted    the mirror case
      a_empty / b_empty   nnz == 0 on one side, three tiles on the other
      tile_cancels_add / _sub   one column, the rows 1..1536 in both: the 512 pairs of tile 1 cancel under + / under -
      columns_cancel_add / _sub  12 columns of 100 pairs: the columns 0, 2, 4, 5, 6, 8 and 11 cancel wholly under + / under -
      total1024, total1025, total2048, total2049   random cells of the first six columns of a 300 x 7 matrix, nnz(A) = total // 2; the last
                     merged element is A's alone, in column 6 (at 1025 and 2049 it is the last tile's only element)
      column_border  8 columns; the merged elements of the columns 0..2 are exactly 1024: column 1 is empty in A, column 2 in B,
                     the columns 3 and 4 in both (either side of the border), column 5 in A, column 6 in B"""
    rng = np.random.default_rng(seed)
    cases = {}
    rows = np.arange(2, 1101)
    ra, rb = np.concatenate([[1], rows]), rows
    va, vb = rng.standard_normal(len(ra)), rng.standard_normal(len(rb))
    A, B, m = _one_column(1200, ra, va, rb, vb)
    cases["split"] = dict(A=A, B=B, m=m, total=2199, split_pairs=[(1023, 1024), (2047, 2048)], split_rows=[513, 1025])
    vb2 = vb.copy()
    vb2[513 - 2] = -va[513 - 1]
    vb2[1025 - 2] = va[1025 - 1]
    A, B, m = _one_column(1200, ra, va, rb, vb2)
    cases["split_cancel"] = dict(A=A, B=B, m=m, total=2199, split_pairs=[(1023, 1024), (2047, 2048)], split_rows=[513, 1025],
                                 cancels={"+": 513, "-": 1025})
    # one operand exhausted inside the first tile
    m = 2000
    small = csc_from_coo(3, np.arange(100), np.zeros(100, np.int64), rng.standard_normal(100))
    bi = np.concatenate([np.arange(49, 1049), np.sort(rng.choice(m, 1500, replace=False)), np.sort(rng.choice(m, 600, replace=False))])
    bj = np.concatenate([np.zeros(1000, np.int64), np.ones(1500, np.int64), np.full(600, 2)])
    large = csc_from_coo(3, bi, bj, rng.standard_normal(3100))
    empty = (np.ones(4, np.int64), np.zeros(0, np.int64), np.zeros(0))
    cases["a_exhausted"] = dict(A=small, B=large, m=m, total=3200, only=(1, [1, 2, 3]))
    cases["b_exhausted"] = dict(A=large, B=small, m=m, total=3200, only=(0, [1, 2, 3]))
    cases["a_empty"] = dict(A=empty, B=large, m=m, total=3100, only=(1, [0, 1, 2, 3]))
    cases["b_empty"] = dict(A=large, B=empty, m=m, total=3100, only=(0, [0, 1, 2, 3]))
    # a whole tile of pairs that cancel
    r = np.arange(1, 1537)
    va = rng.standard_normal(1536)
    for name, sign in (("tile_cancels_add", -1.0), ("tile_cancels_sub", 1.0)):
        vb = rng.standard_normal(1536)
        vb[512:1024] = sign * va[512:1024]
        A, B, m = _one_column(1600, r, va, r, vb)
        cases[name] = dict(A=A, B=B, m=m, total=3072, empty_tiles={"+" if sign < 0 else "-": [1]})
    # whole columns that cancel between kept ones
    gone = [0, 2, 4, 5, 6, 8, 11]
    m = 400
    I = np.concatenate([np.sort(rng.choice(m, 100, replace=False)) for _ in range(12)])
    J = np.repeat(np.arange(12), 100)
    va = rng.standard_normal(1200)
    for name, sign in (("columns_cancel_add", -1.0), ("columns_cancel_sub", 1.0)):
        vb = rng.standard_normal(1200)
        sel = np.isin(J, gone)
        vb[sel] = sign * va[sel]
        cases[name] = dict(A=csc_from_coo(12, I, J, va), B=csc_from_coo(12, I, J, vb), m=m, total=2400,
                           empty_columns={"+" if sign < 0 else "-": gone})
    # totals on the tile size
    for total in (1024, 1025, 2048, 2049):
        ka = total // 2
        ia, ja = _random_cells(rng, 300, 7 - 1, ka - 1)        # (the last column holds the last merged element alone)
        ia, ja = np.append(ia, 299), np.append(ja, 6)
        ib, jb = _random_cells(rng, 300, 7 - 1, total - ka)
        cases["total%d" % total] = dict(A=csc_from_coo(7, ia, ja, rng.standard_normal(ka)),
                                        B=csc_from_coo(7, ib, jb, rng.standard_normal(total - ka)), m=300, total=total)
    # a column change on the tile border
    m = 700
    pick = lambda k: np.sort(rng.choice(m, k, replace=False))
    c0 = rng.permutation(m)[:600]
    c7 = pick(150)
    ia = np.concatenate([np.sort(c0[:300]), pick(224), pick(100), c7])
    ja = np.concatenate([np.zeros(300, np.int64), np.full(224, 2), np.full(100, 6), np.full(150, 7)])
    ib = np.concatenate([np.sort(c0[300:]), pick(200), pick(100), c7])
    jb = np.concatenate([np.zeros(300, np.int64), np.full(200, 1), np.full(100, 5), np.full(150, 7)])
    cases["column_border"] = dict(A=csc_from_coo(8, ia, ja, rng.standard_normal(len(ia))),
                                  B=csc_from_coo(8, ib, jb, rng.standard_normal(len(ib))), m=m, total=1524,
                                  border=(1024, 2, 5), empty_a=[1, 3, 4, 5], empty_b=[2, 3, 4, 6])
    return cases


# ---- whole-wave columns -------------------------------------------------------------------------------------------------------------
WAVE_M, WAVE_N = 700, 64 * 5 + 37
WAVE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 192, 700)
WAVE_LONG = {64: 65, 128 + 5: 128, 128 + 20: 700, 128 + 63: 129, 192 + 1: 127, 192 + 2: 192, WAVE_N - 1: 65}   # column -> length
WAVE_X_SPECIAL = {10: np.inf, 20: np.nan}     # rows of x that only some columns store


def wave_columns(seed=4):
    """700 x 357: the columns of WAVE_LONG are longer than MV_LONG = 64 -- wave 0 has none, wave 1 one at lane 0, wave 2 three
    (lanes 5, 20 and 63; the one at lane 20 is full), wave 3 two neighbours, wave 4 none (every column exactly 64), and the last,
    partly filled wave (37 lanes) the matrix's last column; the other columns cycle through 0, 1, 63 and 64 entries"""
    short = (0, 1, 63, 64)
    lengths = [WAVE_LONG.get(j, 64 if 256 <= j < 320 else short[j % 4]) for j in range(WAVE_N)]
    assert set(lengths) == set(WAVE_LENGTHS)
    return prescribed_lengths(lengths, WAVE_M, seed), lengths


def wave_x(seed=6):
    x = np.random.default_rng(seed).standard_normal(WAVE_M)
    for r, s in WAVE_X_SPECIAL.items():
        x[r] = s
    return x


# ---- the reduction grids ------------------------------------------------------------------------------------------------------------
RED_SIZES = [65537, 262144, 262145, 524289]


def reduction_specials(N):
    """the elements whose loss an off-by-one in the grids would cause: the single element behind the 256th partial (N = 65 537: the
    257th workgroup holds it alone), the first element a second round reads (from 262 145 values on), the last element of that
    round and the element of a third round (524 289); 262 144 fills one round exactly: its last element"""
    return {65537: [65536], 262144: [262143], 262145: [262144], 524289: [262144, 524287, 524288]}[N]


def reduction_vector(N, negative, seed=8):
    """N values of magnitude in [0.5, 1.5] with random signs; the elements of reduction_specials(N) carry 1e3, 2e3, 4e3 (1e-3,
    5e-4, 2.5e-4 for the negative p: there the small values dominate), the largest (smallest) on the last of them"""
    rng = np.random.default_rng(seed + N)
    v = (0.5 + rng.random(N)) * np.where(rng.random(N) < 0.5, -1.0, 1.0)
    for t, i in enumerate(reduction_specials(N)):
        v[i] = -(1e-3 / 2 ** t) if negative else 1e3 * 2 ** t
    return v


def column_vector_csc(v):
    """the N x 1 matrix whose single column is dense"""
    N = len(v)
    return np.array([1, N + 1], np.int64), np.arange(1, N + 1, dtype=np.int64), np.ascontiguousarray(v, np.float64)


GRID_N = MAX_GRID * 256 + 1      # 524 289 segments: the last one is the second round's


def grid_matrix(seed=9):
    """square, n = 524 289: the diagonal and one more entry per column -- the sub-diagonal, except that the columns n-33 .. n-2 have
    theirs in the last row (which holds 33 entries: the only column of the transpose the workgroup sort takes) and the last
    column has it in row n-40.  |values| in [0.5, 1.5], but (n-1, n-1) = 5 and the last column's other entry 3: the largest
    column sum is the last column's, the largest row sum the last row's -- both belong to the second round of a 2048-workgroup grid"""
    n = GRID_N
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.int64)
    extra = j + 1
    extra[n - 33:n - 1] = n - 1
    extra[n - 1] = n - 40
    I = np.concatenate([j, extra])
    J = np.concatenate([j, j])
    V = (0.5 + rng.random(2 * n)) * np.where(rng.random(2 * n) < 0.5, -1.0, 1.0)
    V[n - 1] = 5.0
    V[2 * n - 1] = -3.0
    return csc_from_coo(n, I, J, V), n


# ---- ILU(k): the expansion of a frontier vertex ---------------------------------------------------------------------------------------
FRONTIER_N, FRONTIER_SOURCE, FRONTIER_U1, FRONTIER_U2 = 80, 40, 5, 20


def frontier(width, seed=12):
    """n = 80, a full diagonal.  Column 40 (the source) stores row 5; column 5 stores exactly `width` rows: itself, row 20 and
    width - 2 rows beyond 40 -- at K >= 1 these become level-1 fill of column 40; column 20 stores exactly `width` rows: itself and
    width - 1 rows beyond 40, half of them column 5's -- at K >= 2 the others become level-2 fill of column 40.  The columns 60 and
    70 store the rows 5 and 20 as well (more sources that reach the two vertices).  Diagonal 8 + U(0, 1), the rest 0.1 * normal.
    -> (the CSC arrays, those of its transpose: the upper search walks the same frontier there), rows of column 5, of column 20"""
    n, src, u1, u2 = FRONTIER_N, FRONTIER_SOURCE, FRONTIER_U1, FRONTIER_U2
    rng = np.random.default_rng(seed + width)
    beyond = np.arange(src + 1, n)
    r1 = np.sort(rng.choice(beyond, width - 2, replace=False))
    half = (width - 1) // 2
    r2 = np.sort(np.concatenate([r1[:half], rng.choice(np.setdiff1d(beyond, r1), width - 1 - half, replace=False)]))
    I = np.concatenate([np.arange(n), [u1], [u2], r1, r2, [u1, u2]])
    J = np.concatenate([np.arange(n), [src], [u1], np.full(len(r1), u1), np.full(len(r2), u2), [60, 70]])
    V = np.concatenate([8.0 + rng.random(n), 0.1 * rng.standard_normal(len(I) - n)])
    csc = csc_from_coo(n, I, J, V)
    return csc, transpose_csc(n, csc), r1, r2
