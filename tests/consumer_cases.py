"""Deterministic cases for the readers and editors of the assembled CSC (csrc/consumers.hip): dropzeros!, getindex, the pending
buffer's getindex, the row-wise index behind mul! / opnorm(A, Inf), the Dirichlet helpers and the diagonal set-up.

numpy only: no GPU, no oracle.  A matrix is a Case (name, m, n, colptr, rowval, nzval) with Julia's 1-based arrays, installed on
the device with `A.cscmatrix = esp.SparseMatrixCSC(...)` and in the oracle with `orc.CSC(m, n, colptr, rowval, nzval)` -- the only
way to a stored -0.0, NaN or exact zero at a chosen position.  Every builder returns (case or stream, props); props says what the
case claims about itself, and tests/test_consumer_cases.py checks every claim before tests/test_consumers_gpu.py relies on it.

The constants below restate what the kernels are built around.  source_constants() reads them from the sources, so that a change
there fails the CPU test instead of moving a GPU test off its edge without anybody noticing.
"""
import collections
import os
import re

import numpy as np

SET, UPDATE, RAWUPDATE = 0, 1, 2
SCAN_CHUNK = 2048          # flags per workgroup of the scan behind dropzeros! (scan.hpp: THREADS * ITEMS)
SORT_TILE = 4096           # entries per tile of the row sort of build_csr (radix.hpp: THREADS * ITEMS)
SORT_PASS_BITS = 8         # row bits per pass of that sort (partition.hip, sort_segment_lsd: done += 8)
PENDING_MATCH_CAP = 2048   # matches esp_pending_getindex folds (consumers.hip)
PENDING_FOLD_THREADS = 256  # stride of the rank sort of pending_fold_k
PENDING_MAX_GROUPS = 4096  # workgroups of pending_matches_k, 256 threads each
LAZY_COLPTR_N = 4096       # reset! leaves colptr := 1 to the next reader for n above this (handle.hip: init_empty_csc)
PENALTY = 1.0e20           # mark_dirichlet's default

Case = collections.namedtuple("Case", "name m n colptr rowval nzval")

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "extendablesparse.jl_amd", "csrc")


def _const(text, name, namespace=None):
    if namespace is not None:
        text = text[text.index("namespace %s" % namespace):]
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def source_constants():
    """The same constants as the sources state them"""
    def read(f):
        with open(os.path.join(_CSRC, f)) as fh:
            return fh.read()
    scan, radix, cons, handle, part = read("scan.hpp"), read("radix.hpp"), read("consumers.hip"), read("handle.hip"), read("partition.hip")
    # build_csr sorts its Z entries on the h->L.rb row bits by the one driver of partition.hip: the pass width read below is its loop's
    assert re.search(r"sort_segment_lsd\(h, [^;]*, Z, 0, h->L\.rb, ", cons), "build_csr no longer sorts by sort_segment_lsd"
    return dict(
        SCAN_CHUNK=_const(scan, "THREADS", "espscan") * _const(scan, "ITEMS", "espscan"),
        SORT_TILE=_const(radix, "THREADS", "espradix") * _const(radix, "ITEMS", "espradix"),
        SORT_PASS_BITS=int(re.search(r"done < bits; done \+= (\d+),", part).group(1)),
        PENDING_MATCH_CAP=_const(cons, "PENDING_MATCH_CAP"),
        PENDING_FOLD_THREADS=int(re.search(r"q < n; q \+= (\d+)\)", cons).group(1)),
        PENDING_MAX_GROUPS=int(re.search(r"std::min<i64>\((\d+), std::max<i64>\(1, ceil_div<i64>\(h->count, 256\)\)\)", cons).group(1)),
        LAZY_COLPTR_N=int(re.search(r"!windowed\(h\) && h->n > (\d+)\)", handle).group(1)),
    )


def bits_for(extent):
    """common.hpp: bits needed for 0 .. extent-1, at least 1 (the row bits of a matrix with `extent` rows)"""
    b = 1
    while (1 << b) < extent:
        b += 1
    return b


def sort_passes(m):
    """(bits of every pass) of build_csr's row sort for a matrix with m rows"""
    rb = bits_for(m)
    return [min(SORT_PASS_BITS, rb - done) for done in range(0, rb, SORT_PASS_BITS)]


def csc_from_coo(name, m, n, rows, cols, vals):
    """A Case from distinct 1-based positions (any order)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float64)
    assert len(rows) == len(cols) == len(vals)
    if len(rows):
        assert rows.min() >= 1 and rows.max() <= m and cols.min() >= 1 and cols.max() <= n
    key = (cols - 1) * m + (rows - 1)
    order = np.argsort(key, kind="stable")
    assert len(np.unique(key)) == len(key), "positions must be distinct"
    colptr = np.ones(n + 1, np.int64)
    colptr[1:] += np.cumsum(np.bincount(cols - 1, minlength=n))
    return Case(name, int(m), int(n), colptr, rows[order].copy(), vals[order].copy())


def coo_of(case):
    """(rows, cols) of every stored entry, 1-based, in storage order"""
    cols = np.repeat(np.arange(1, case.n + 1, dtype=np.int64), np.diff(case.colptr))
    return case.rowval.copy(), cols


def _random_positions(rng, m, n, Z, cols=None):
    """Z distinct positions of an m x n matrix (columns restricted to `cols`, 0-based, if given)"""
    cols = np.arange(n) if cols is None else np.asarray(cols)
    assert Z <= m * len(cols)
    flat = rng.choice(m * len(cols), size=Z, replace=False)
    return flat % m + 1, cols[flat // m] + 1


def _nonzero_values(rng, Z):
    v = rng.standard_normal(Z)
    v[v == 0.0] = 1.0
    return v


# ------------------------------------------------------------------------------------------------------------ dropzeros!
DROP_Z = (1, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 3 * SCAN_CHUNK + 5)
DROP_SETS = ("none", "all", "first", "last", "alternate")
SPECIAL_VALUES = (0.0, -0.0, float("nan"), 5e-324, 1.5, float("-inf"))


def _zero_set(which, Z):
    z = np.zeros(Z, bool)
    if which == "all":
        z[:] = True
    elif which == "first":
        z[0] = True
    elif which == "last":
        z[-1] = True
    elif which == "alternate":
        z[::2] = True
    elif which != "none":
        raise ValueError(which)
    return z


def drop_props(case):
    """What dropzeros! has to do with a case: the dropped indices, the scan chunks they lie in, the columns that become empty"""
    zero = case.nzval == 0.0
    drop = np.flatnonzero(zero)
    _, cols = coo_of(case)
    before = np.diff(case.colptr)
    after = np.bincount(cols[~zero] - 1, minlength=case.n)
    return dict(Z=len(case.nzval), drop=drop, kept=int((~zero).sum()), chunks=sorted(set((drop // SCAN_CHUNK).tolist())),
                emptied=np.flatnonzero((before > 0) & (after == 0)) + 1, empty_before=np.flatnonzero(before == 0) + 1)


def drop_case(Z, which, seed=1):
    """Z entries spread over a 97 x 101 matrix, the zero set `which` of DROP_SETS (Z = 1: one entry, dropped or not)"""
    rng = np.random.default_rng([seed, Z, DROP_SETS.index(which)])
    m, n = 97, 101
    r, c = _random_positions(rng, m, n, Z)
    case = csc_from_coo("drop_Z%d_%s" % (Z, which), m, n, r, c, _nonzero_values(rng, Z))
    case.nzval[_zero_set(which, Z)] = 0.0
    return case, drop_props(case)


def drop_chunk_edges(seed=2):
    """3 * 2048 + 5 entries; dropped: index 0, the three indices around every chunk boundary (2047, 2048, 2049, 4095, ...) and
    the last entry -- a kept entry on either side of every run of drops"""
    Z = 3 * SCAN_CHUNK + 5
    rng = np.random.default_rng([seed, 3])
    r, c = _random_positions(rng, 97, 101, Z)
    case = csc_from_coo("drop_chunk_edges", 97, 101, r, c, _nonzero_values(rng, Z))
    idx = [0, Z - 1] + [b * SCAN_CHUNK + d for b in (1, 2, 3) for d in (-1, 0, 1)]
    case.nzval[idx] = 0.0
    return case, drop_props(case)


def drop_random_empty_columns(seed=3):
    """35 % zeros at random over 3 * 2048 + 5 entries of a 97 x 120 matrix whose columns 1-5, 51-60 and 116-120 are empty;
    column 77 holds zeros only (it becomes empty), its neighbours do not"""
    Z, m, n = 3 * SCAN_CHUNK + 5, 97, 120
    rng = np.random.default_rng([seed, 5])
    cols = np.array([c for c in range(n) if not (c < 5 or 50 <= c < 60 or c >= 115)])
    r, c = _random_positions(rng, m, n, Z, cols)
    case = csc_from_coo("drop_random_empty_columns", m, n, r, c, _nonzero_values(rng, Z))
    case.nzval[rng.random(Z) < 0.35] = 0.0
    a, b = case.colptr[76] - 1, case.colptr[77] - 1
    case.nzval[a:b] = 0.0
    for col in (76, 78):
        a, b = case.colptr[col - 1] - 1, case.colptr[col] - 1
        case.nzval[a] = 2.5
    return case, drop_props(case)


def drop_special_values(seed=4):
    """values drawn from {0.0, -0.0, NaN, 5e-324, 1.5, -Inf} over 2 * 2048 + 77 entries: both zeros go, the rest stays"""
    Z = 2 * SCAN_CHUNK + 77
    rng = np.random.default_rng([seed, 7])
    r, c = _random_positions(rng, 97, 101, Z)
    case = csc_from_coo("drop_special_values", 97, 101, r, c, np.array(SPECIAL_VALUES)[rng.integers(0, 6, Z)])
    case.nzval[:6] = SPECIAL_VALUES      # (every value at least once)
    return case, drop_props(case)


def drop_rectangular(shape, seed=5):
    """"row": 1 x 2500, "column": 2500 x 1; two thirds of the positions stored, every third stored value 0.0 or -0.0"""
    rng = np.random.default_rng([seed, 9])
    L = 2500
    pos = np.flatnonzero(rng.random(L) < 0.66) + 1
    v = _nonzero_values(rng, len(pos))
    v[::3] = 0.0
    v[1::6] = -0.0
    one = np.ones(len(pos), np.int64)
    if shape == "row":
        case = csc_from_coo("drop_1xn", 1, L, one, pos, v)
    else:
        case = csc_from_coo("drop_mx1", L, 1, pos, one, v)
    return case, drop_props(case)


def drop_cases():
    """name -> (case, props): every dropzeros! case"""
    out = {}
    for Z in DROP_Z:
        for which in DROP_SETS:
            case, p = drop_case(Z, which)
            out[case.name] = (case, p)
    for case, p in (drop_chunk_edges(), drop_random_empty_columns(), drop_special_values(), drop_rectangular("row"),
                    drop_rectangular("column")):
        out[case.name] = (case, p)
    return out


def join_stream(case, count=300, seed=6):
    """UPDATE / RAWUPDATE / SET calls for the flush after dropzeros!: a third at positions dropzeros! removed (where there are any),
    a third at positions it kept, a third at positions never stored -- with zeros among the values"""
    rng = np.random.default_rng([seed, len(case.nzval), case.m])
    r, c = coo_of(case)
    zero = case.nzval == 0.0
    I, J = [], []
    for sel in (np.flatnonzero(zero), np.flatnonzero(~zero)):
        if len(sel):
            pick = rng.choice(sel, size=count // 3)
            I.append(r[pick])
            J.append(c[pick])
    ci, cj = rng.integers(1, case.m + 1, 20 * count), rng.integers(1, case.n + 1, 20 * count)
    fresh = np.flatnonzero(~np.isin((cj - 1) * case.m + ci - 1, (c - 1) * case.m + r - 1))[:count // 3]
    I.append(ci[fresh])
    J.append(cj[fresh])
    I, J = np.concatenate(I), np.concatenate(J)
    order = rng.permutation(len(I))
    I, J = I[order], J[order]
    V = rng.standard_normal(len(I))
    V[rng.random(len(I)) < 0.15] = 0.0
    kinds = rng.integers(0, 3, len(I)).astype(np.uint8)
    return kinds, I, J, V


# -------------------------------------------------------------------------------------------------------------- getindex
GETINDEX_COLUMN_TYPES = ("empty", "one", "two", "three", "sixty_four", "dense")


def getindex_case(seed=7):
    """200 rows; columns of every type, an empty one first, last and in the middle: 1 entry (at row 1, at row m, inside), 2, 3, 64
    and all 200 rows stored.  Column 4 stores 0.0 and -0.0."""
    m = 200
    rng = np.random.default_rng([seed, 11])
    columns = [[], [1], [m], [57], [40, 41], [1, m], [2, 100, 199], [1, 2, 3], sorted(rng.choice(m, 64, replace=False) + 1), [],
               list(range(1, m + 1)), [3, 5, 7], sorted(rng.choice(m, 64, replace=False) + 1), list(range(1, m + 1)), []]
    rows = np.array([r for col in columns for r in col], np.int64)
    cols = np.array([j + 1 for j, col in enumerate(columns) for _ in col], np.int64)
    vals = _nonzero_values(rng, len(rows))
    case = csc_from_coo("getindex", m, len(columns), rows, cols, vals)
    a = case.colptr[4] - 1                      # column 5 = [40, 41]
    case.nzval[a], case.nzval[a + 1] = 0.0, -0.0
    case.nzval[case.colptr[10] - 1 + 99] = 0.0  # inside the first dense column (row 100)
    types = {0: "empty", 1: "one", 2: "two", 3: "three", 64: "sixty_four", m: "dense"}
    return case, dict(types=[types[len(c)] for c in columns], zero_at=(40, 5), negzero_at=(41, 5), dense_zero_at=(100, 11))


def getindex_lookups(case):
    """(i, j) for every column: the first and the last stored row, every stored row of a column of up to 3, the rows just below
    and above every one of those, rows 1 and m"""
    out = []
    for j in range(1, case.n + 1):
        rows = case.rowval[case.colptr[j - 1] - 1: case.colptr[j] - 1]
        want = {1, case.m}
        probe = list(rows) if len(rows) <= 3 else [rows[0], rows[-1], rows[len(rows) // 2]]
        for r in probe:
            want |= {int(r) - 1, int(r), int(r) + 1}
        out += [(i, j) for i in sorted(want) if 1 <= i <= case.m]
    return out


# ------------------------------------------------------------------------------------------------ getindex of the pending buffer
PENDING_M, PENDING_N = 50, 60
PENDING_TARGET = (23, 41)
PENDING_NOISE = 200000
PENDING_K = (1, 255, 256, 257, 2047, 2048)
PENDING_VALUES = (0.0, -0.0, 1.0, 2.0 ** -60, -1e300, 1e300)


def fold(kinds, vals, present=False, acc=0.0):
    """The state machine of csrc/fold.hpp (fold_step) over calls at ONE position in IEEE double arithmetic: (present, value)"""
    for k, v in zip(np.asarray(kinds).tolist(), np.asarray(vals, np.float64).tolist()):
        if k == SET:
            if present or v != 0.0:
                present, acc = True, v
        elif present:
            acc = acc + v
        elif k == RAWUPDATE or v != 0.0:
            present, acc = True, 0.0 + v
    return present, (acc if present else 0.0)


def target_calls(k, seed=8):
    """(kinds, vals) of the k calls at the target (k = 1 or k >= 16), kinds SET / UPDATE / RAWUPDATE mixed and values from
    PENDING_VALUES, built so that the result depends on the order of the calls as far as floating point allows it:

      head
        UPDATE 0.0      creates nothing (RAWUPDATE would)
        SET -0.0        creates nothing
        RAWUPDATE 1e300 creates the position
        UPDATE 1.0      absorbed
        UPDATE -1e300   back to exactly 0.0: one step later and the 1.0 would count, one step earlier and the entry is -1e300
        SET 2^-60       on a present position: whatever comes before it is gone, whatever comes after is not
      body
        UPDATE and RAWUPDATE of 2^-60 (the first 40: exact sums), then of 1.0, 2^-60, 0.0 and -0.0 at random: the sum counts the
        1.0s that arrive and rounds differently when a 2^-60 arrives at another place

    A swap of two neighbours CANNOT change the result of every such sequence: x + 0.0 == x and x + -0.0 == x for every stored x, a
    SET or a +-1e300 erases what came before it, and sums that stay exact commute -- the literal "every neighbour swap" is out of
    reach for any sequence over these kinds and values.  What the sequences do guarantee (tests/test_consumer_cases.py folds each
    variant): the swap of the head's -1e300 and SET changes the result; so do the reversed order, every shuffled order, a lost
    and a doubled 1.0, and matches folded in the order of a rank sort that handles its first 256 elements only.
    k = 1: RAWUPDATE -0.0 -- the position exists afterwards and holds 0.0 + -0.0 = +0.0."""
    assert k == 1 or k >= 16
    rng = np.random.default_rng([seed, k])
    T = 2.0 ** -60
    if k == 1:
        calls = [(RAWUPDATE, -0.0)]
    else:
        head = [(UPDATE, 0.0), (SET, -0.0), (RAWUPDATE, 1e300), (UPDATE, 1.0), (UPDATE, -1e300), (SET, T)]
        nb = k - len(head)
        kinds = rng.choice([UPDATE, RAWUPDATE], nb)
        vals = np.array([1.0, T, 0.0, -0.0])[rng.choice(4, nb, p=[0.45, 0.35, 0.1, 0.1])]
        vals[:min(40, nb)] = T
        calls = head + list(zip(kinds.tolist(), vals.tolist()))
    kinds = np.array([c[0] for c in calls], np.uint8)
    vals = np.array([c[1] for c in calls], np.float64)
    assert len(kinds) == k
    return kinds, vals


def pending_stream(k, seed=9, noise=PENDING_NOISE, target=PENDING_TARGET):
    """`noise` calls at random positions other than the target of a 50 x 60 matrix with the k calls of target_calls(k) at random
    places among them (their order kept): (kinds, I, J, V), props"""
    rng = np.random.default_rng([seed, k])
    E = noise + k
    I = rng.integers(1, PENDING_M + 1, E)
    J = rng.integers(1, PENDING_N + 1, E)
    hit = (I == target[0]) & (J == target[1])
    I[hit] = target[0] % PENDING_M + 1      # (never the target)
    kinds = rng.integers(0, 3, E).astype(np.uint8)
    V = np.array(PENDING_VALUES)[rng.integers(0, 6, E)]
    V[rng.random(E) < 0.5] = 1.0            # (finite sums at most positions)
    at = np.sort(rng.choice(E, size=k, replace=False)) if k else np.empty(0, np.int64)
    tk, tv = target_calls(k) if k else (np.empty(0, np.uint8), np.empty(0))
    I[at], J[at], kinds[at], V[at] = target[0], target[1], tk, tv
    return (kinds, I, J, V), dict(at=at, target=target, groups=min(PENDING_MAX_GROUPS, -(-E // 256)))


# ----------------------------------------------------------------------------------------- mul! and the row-wise index
MUL_M = (1, 2, 255, 256, 257, 65536, 65537, 2 ** 24 + 1)
MUL_Z = (0, 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1)


def mul_rows_case(m, seed=10):
    """about 5000 entries over m rows (2^24 + 1 rows: 7 columns, 300 entries); rows 1 and m are stored in six columns each, so the
    lowest and the highest row bit both decide an order"""
    rng = np.random.default_rng([seed, m])
    if m > 1 << 20:
        n, Z = 7, 300
    else:
        n, Z = max(64, -(-6000 // m)), 5000
    r, c = _random_positions(rng, m, n, Z)
    edge = np.arange(1, 7)
    r = np.concatenate([r, np.full(6, m), np.ones(6, np.int64)])
    c = np.concatenate([c, edge, edge])
    _, first = np.unique((c - 1) * m + r - 1, return_index=True)
    r, c = r[first], c[first]
    case = csc_from_coo("mul_m%d" % m, m, n, r, c, rng.standard_normal(len(r)))
    return case, dict(row_bits=bits_for(m), passes=sort_passes(m))


def mul_count_case(Z, seed=11):
    """Z entries in a 300 x 200 matrix"""
    rng = np.random.default_rng([seed, Z])
    r, c = _random_positions(rng, 300, 200, Z)
    return csc_from_coo("mul_Z%d" % Z, 300, 200, r, c, rng.standard_normal(Z)), dict(tiles=-(-Z // SORT_TILE))


def mul_one_row(seed=12):
    """300 x 9000, row 137 full and nothing else: one row longer than two sort tiles"""
    rng = np.random.default_rng([seed, 13])
    n = 9000
    return csc_from_coo("mul_one_row", 300, n, np.full(n, 137), np.arange(1, n + 1), rng.standard_normal(n)), dict(row=137)


def mul_dense_column(seed=13):
    """5000 x 40: column 17 dense, 600 entries elsewhere"""
    rng = np.random.default_rng([seed, 15])
    m, n = 5000, 40
    r, c = _random_positions(rng, m, n, 600, [j for j in range(n) if j != 16])
    r = np.concatenate([r, np.arange(1, m + 1)])
    c = np.concatenate([c, np.full(m, 17)])
    return csc_from_coo("mul_dense_column", m, n, r, c, rng.standard_normal(len(r))), dict(column=17)


def mul_empty_edge_rows(seed=14):
    """700 x 90, 4000 entries, rows 1 and 700 empty (and row 350)"""
    rng = np.random.default_rng([seed, 17])
    r, c = _random_positions(rng, 700, 90, 4000)
    keep = (r != 1) & (r != 700) & (r != 350)
    return csc_from_coo("mul_empty_edge_rows", 700, 90, r[keep], c[keep], rng.standard_normal(int(keep.sum()))), dict(empty=(1, 350, 700))


NONFINITE_STRIDES = ((7, float("inf")), (11, float("-inf")), (13, float("nan")))


def mul_nonfinite(seed=15):
    """(case, x): 400 x 300 with 5000 entries; x holds Inf at every 7th column, -Inf at every 11th, NaN at every 13th (the later
    stride wins), and the matrix stores 0.0 and -0.0 in those columns: 0 * Inf is NaN, a kernel that skipped stored zeros would
    give a finite row.  Rows 391 .. 400 hold stored zeros at non-finite columns ONLY."""
    rng = np.random.default_rng([seed, 19])
    m, n = 400, 300
    x = rng.standard_normal(n)
    for stride, v in NONFINITE_STRIDES:
        x[stride - 1::stride] = v
    special = np.flatnonzero(~np.isfinite(x))
    r, c = _random_positions(rng, 390, n, 5000)
    vals = rng.standard_normal(5000)
    at_special = np.isin(c - 1, special)
    z = at_special & (rng.random(5000) < 0.6)
    vals[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    # the rows that hold nothing but stored zeros at non-finite columns
    rr = np.repeat(np.arange(391, 401), 3)
    cc = special[np.arange(30) % len(special)] + 1
    vv = np.where(np.arange(30) % 2 == 0, 0.0, -0.0)
    case = csc_from_coo("mul_nonfinite", m, n, np.concatenate([r, rr]), np.concatenate([c, cc]), np.concatenate([vals, vv]))
    return (case, x), dict(special=special + 1, zero_rows=np.arange(391, 401))


def mul_negzero(seed=16):
    """(case, x): 64 x 50; the products of rows 1 .. 32 are all -0.0 (-v * 0.0, 0.0 * -u, -0.0 * u): r[i] = 0.0 + -0.0 + ... = +0.0"""
    rng = np.random.default_rng([seed, 21])
    m, n = 64, 50
    x = np.abs(rng.standard_normal(n)) + 0.5
    x[::2] = 0.0
    x[1::4] = -x[1::4]
    r, c = _random_positions(rng, m, n, 1200)
    vals = np.abs(rng.standard_normal(1200)) + 0.5
    low = r <= 32
    xc = x[c - 1]
    vals[low & (xc == 0.0)] *= -1.0             # -v * +0.0 = -0.0
    vals[low & (xc < 0.0)] = 0.0                # +0.0 * -u = -0.0
    vals[low & (xc > 0.0)] = -0.0               # -0.0 * +u = -0.0
    return (csc_from_coo("mul_negzero", m, n, r, c, vals), x), dict(rows=np.arange(1, 33))


def mul_cases():
    """name -> (case, props) for the cases that take any x"""
    out = {}
    for m in MUL_M:
        case, p = mul_rows_case(m)
        out[case.name] = (case, p)
    for Z in MUL_Z:
        case, p = mul_count_case(Z)
        out[case.name] = (case, p)
    for case, p in (mul_one_row(), mul_dense_column(), mul_empty_edge_rows()):
        out[case.name] = (case, p)
    out["mul_n0"] = (Case("mul_n0", 5, 0, np.ones(1, np.int64), np.empty(0, np.int64), np.empty(0)), dict())
    out["mul_m0"] = (Case("mul_m0", 0, 5, np.ones(6, np.int64), np.empty(0, np.int64), np.empty(0)), dict())
    return out


def mul_x(case, seed=17):
    return np.random.default_rng([seed, case.n, case.m % 1000]).standard_normal(case.n)


# ------------------------------------------------------------------------------------------- every editor x every reader
EDITOR_N = 5000
EDITORS = ("flush_hits", "flush_adds", "set_nzval", "zero_values", "eliminate_dirichlet", "dropzeros_drops", "dropzeros_nothing",
           "diag_scale_inplace", "set_csc", "set_csc_i32", "reset", "release", "sum_home")
# what the editor does to a preconditioner made before it: "pattern" -- ldiv! refuses; "values" -- it answers with its old diagonal
EDITOR_EFFECT = dict(flush_hits="values", flush_adds="pattern", set_nzval="values", zero_values="values", eliminate_dirichlet="values",
                     dropzeros_drops="pattern", dropzeros_nothing="values", diag_scale_inplace="values", set_csc="pattern",
                     set_csc_i32="pattern", reset="pattern", release="pattern", sum_home="pattern")


def editor_base(zeros=True, seed=18, n=EDITOR_N):
    """n x n with n = 5000 (above the lazy-colptr threshold): a diagonal in nine columns of ten, three off-diagonal entries per
    column on average, every 50th diagonal at or above the Dirichlet penalty; zeros=True stores 0.0 at every 9th entry"""
    rng = np.random.default_rng([seed, 23])
    r, c = _random_positions(rng, n, n, 3 * n)
    off = r != c
    d = np.flatnonzero(np.arange(n) % 10 != 3) + 1
    r, c = np.concatenate([r[off], d]), np.concatenate([c[off], d])
    vals = _nonzero_values(rng, len(r))
    case = csc_from_coo("editor_base_zeros" if zeros else "editor_base", n, n, r, c, vals)
    rr, cc = coo_of(case)
    diag = np.flatnonzero(rr == cc)
    case.nzval[diag] = np.abs(case.nzval[diag]) + 2.0
    case.nzval[diag[::50]] = PENALTY
    case.nzval[diag[25::50]] = 3.0e20
    if zeros:
        case.nzval[4::9] = 0.0
    return case, dict(diag=diag, marked=int((case.nzval[diag] >= PENALTY).sum()))


def editor_other(seed=19, n=EDITOR_N):
    """another n x n matrix (two entries per column, no relation to editor_base): what the cscmatrix setters install"""
    rng = np.random.default_rng([seed, 25])
    r, c = _random_positions(rng, n, n, 2 * n)
    return csc_from_coo("editor_other", n, n, r, c, _nonzero_values(rng, 2 * n)), dict()


def editor_hits(case, count=4000, seed=20):
    """UPDATE calls at stored positions only (duplicates among them)"""
    rng = np.random.default_rng([seed, 27])
    r, c = coo_of(case)
    pick = rng.integers(0, len(r), count)
    return np.full(count, UPDATE, np.uint8), r[pick], c[pick], rng.standard_normal(count)


def editor_adds(case, count=4000, seed=21):
    """RAWUPDATE calls at random positions: most of them are not stored yet"""
    rng = np.random.default_rng([seed, 29])
    return (np.full(count, RAWUPDATE, np.uint8), rng.integers(1, case.m + 1, count), rng.integers(1, case.n + 1, count),
            rng.standard_normal(count))


def stored_fraction(case, I, J):
    key = set(((coo_of(case)[1] - 1) * case.m + coo_of(case)[0] - 1).tolist())
    return float(np.mean([((j - 1) * case.m + i - 1) in key for i, j in zip(I.tolist(), J.tolist())]))


READERS = ("mul", "opnorm_inf", "jacobi", "mark_dirichlet", "getindex", "pattern_hash", "copy", "transpose", "norm", "issymmetric",
           "arrays")
WINDOW = (1001, 2000)      # the column window of the lazy-tail state (1-based, inclusive), n = EDITOR_N


def window_stream(seed=22, n=EDITOR_N, count=3000):
    """RAWUPDATE calls whose columns lie inside WINDOW"""
    rng = np.random.default_rng([seed, 31])
    return (np.full(count, RAWUPDATE, np.uint8), rng.integers(1, n + 1, count), rng.integers(WINDOW[0], WINDOW[1] + 1, count),
            _nonzero_values(rng, count))


def diagonal_case(n, seed=23):
    """n x n with one stored diagonal entry per column, every one above the Dirichlet penalty (1e20 * j): what reset! has to make
    forget -- a reader that met the old colptr would still find a marked diagonal in every column"""
    idx = np.arange(1, n + 1)
    return csc_from_coo("diagonal_%d" % n, n, n, idx, idx, PENALTY * idx), dict()


# -------------------------------------------------------------------------------------- Dirichlet helpers, diagonal set-up
DIRICHLET_N = (1, 255, 256, 257)


def dirichlet_case(n, full_diagonal=False, seed=24):
    """n x n.  Per column: the diagonal (unless the column is one of those without), up to four off-diagonal entries.  Diagonals:
    exactly the penalty (j % 8 == 0), above it (j % 8 == 4), NaN (j % 16 == 5), 0.0 (j % 16 == 6), -0.0 (j % 16 == 7), missing
    (j % 16 == 9 and j % 16 == 13; none with full_diagonal), else ordinary.  Off-diagonal: one entry of 7e20 -- above the penalty -- per
    eight columns, stored zeros at every 5th, and every marked node has entries in its row AND its column.  n = 1: the diagonal
    alone, exactly the penalty."""
    rng = np.random.default_rng([seed, n, int(full_diagonal)])
    j = np.arange(1, n + 1)
    if n == 1:
        return csc_from_coo("dirichlet_1", 1, 1, [1], [1], [PENALTY]), dict(missing=np.empty(0, np.int64), marked=np.array([1]))
    missing = np.empty(0, np.int64) if full_diagonal else j[(j % 16 == 9) | (j % 16 == 13)]
    dj = np.setdiff1d(j, missing)
    dv = 1.0 + np.abs(rng.standard_normal(len(dj)))
    dv[dj % 8 == 0] = PENALTY
    dv[dj % 8 == 4] = 2.5e20
    if not full_diagonal:
        dv[dj % 16 == 5] = np.nan
        dv[dj % 16 == 6] = 0.0
        dv[dj % 16 == 7] = -0.0
    r, c = _random_positions(rng, n, n, 4 * n)
    off = r != c
    r, c = r[off], c[off]
    ov = _nonzero_values(rng, len(r))
    ov[::5] = 0.0
    ov[3::8 * 4] = 7e20
    # a neighbour above and below every marked node, in its column and in its row
    mk = dj[(dj % 8 == 0) | (dj % 8 == 4)]
    er = np.concatenate([np.clip(mk - 1, 1, n), np.clip(mk + 1, 1, n), mk, mk])
    ec = np.concatenate([mk, mk, np.clip(mk - 1, 1, n), np.clip(mk + 1, 1, n)])
    ok = er != ec
    rows, cols = np.concatenate([dj, r, er[ok]]), np.concatenate([dj, c, ec[ok]])
    vals = np.concatenate([dv, ov, np.full(int(ok.sum()), 0.75)])
    key = (cols - 1) * n + rows - 1
    _, first = np.unique(key, return_index=True)
    case = csc_from_coo("dirichlet_%d%s" % (n, "_full" if full_diagonal else ""), n, n, rows[first], cols[first], vals[first])
    return case, dict(missing=missing, marked=mk)


def diagonal_of(case):
    """(stored, value) per column: whether (j, j) is stored, and its value"""
    r, c = coo_of(case)
    d = r == c
    stored = np.zeros(case.n, bool)
    val = np.zeros(case.n)
    stored[c[d] - 1] = True
    val[c[d] - 1] = case.nzval[d]
    return stored, val
