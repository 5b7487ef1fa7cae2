"""Deterministic update streams for the PAIR form of the small bucket kernel (csrc/local_w.hip: pair_k, pair_pred_k).

numpy only: no GPU, no oracle.  Every builder returns (Stream, props): the stream is (m, n, kind, I, J, V) with J ascending
(1-based indices, so that an append on an empty buffer is the partition and leaves a RawPlan), props a small dict of what
the stream claims about itself -- tests/test_pair_streams.py checks every claim with numpy and the oracle before a GPU test
relies on it.  The repeat_* builders return (m, n, kind, [(I, J, V), ...], props): batches over the same J.

What the host asks before it chooses the pair kernel (csrc/flush.hip, pair_ok) and what the streams therefore keep:
  one kind | count <= 12 n | buckets of <= 256 columns and <= 3072 entries | fewer than 32 row bits | count > 4096.
The plan (csrc/partition.hip, plan_prefix_bits) cuts buckets of 2^c columns for the smallest prefix with
count / n * 2^c <= 0.9 * 4096: 256-column buckets for an average of more than 7.2 and at most 12 entries per column, and -- the
prefix must have more than 8 bits -- more than 2^16 columns.  A later flush of the same handle takes one prefix bit less when the
fullest bucket would still fit twice (2 * longest bucket <= 0.98 * 4096): the streams hold one pair of buckets filled to the brim
(512 columns x 12), so that the cut stays at 256 columns.
"""
import collections

import numpy as np

SET, UPDATE, RAWUPDATE, COO = 0, 1, 2, 3
BUCKET, PAIR, RUN = 256, 512, 12       # columns of a producer bucket, of a pair; the longest column run the pair kernel takes
BUCKET_ENTRIES = 3072                  # the small variant's segment capacity
ROW_SPAN = 1 << 19                     # rows of a pair must span less than this
PLAN_TARGET = 0.9 * 4096               # entries the plan puts into a bucket on average, at most

Stream = collections.namedtuple("Stream", "m n kind I J V")


def plan_cap_for(density, cols):
    """The esp_debug_plan_cap value that makes the FIRST flush of a handle cut buckets of `cols` (a power of two) columns for a
    stream of `density` entries per column: density * cols <= cap < density * 2 * cols (the geometric middle)."""
    return density * cols * 2.0 ** 0.5


def oracle_csc(orc, m, n, kind, I, J, V, sub=False):
    """(colptr, rowval, nzval) of the stream applied to an empty m x n matrix by the CPU oracle `orc` (the module oracle/oracle.py,
    passed in: this file imports none); sub: the append's op is "-" (every kind but SET takes -v)"""
    if sub and kind != SET:
        V = -np.asarray(V, np.float64)
    if kind == COO:
        return orc.sparse_coo(I, J, V, m, n).arrays()
    O = orc.ExtendableSparseMatrix(m, n)
    O.apply(np.full(len(I), kind, np.uint8), I, J, V)
    O.flush()
    return O.arrays()


def _expand(L):
    """J (ascending, 1-based) and every entry's index inside its column, for the run lengths L"""
    L = np.asarray(L, np.int64)
    J = np.repeat(np.arange(1, len(L) + 1, dtype=np.int64), L)
    q = np.arange(len(J), dtype=np.int64) - np.repeat(np.cumsum(L) - L, L)
    return J, q


def _blocks(n, J, width=PAIR):
    return (np.asarray(J) - 1) // width, (n + width - 1) // width


def describe(m, n, I, J):
    """What a stream is, measured: longest run, density, wholly empty 256- and 512-column blocks, row span of every 512-column
    block (-1 where it is empty) and the entries of the fullest 256-column block."""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    runs = np.bincount(J - 1, minlength=n)
    out = dict(maxrun=int(runs.max()) if n else 0, density=len(J) / float(n))
    for name, width in (("empty_buckets", BUCKET), ("empty_pairs", PAIR)):
        b, nb = _blocks(n, J, width)
        out[name] = np.flatnonzero(np.bincount(b, minlength=nb) == 0).tolist()
    b, nb = _blocks(n, J, PAIR)
    lo = np.full(nb, np.iinfo(np.int64).max)
    hi = np.full(nb, -1)
    np.minimum.at(lo, b, I)
    np.maximum.at(hi, b, I)
    out["pair_span"] = np.where(hi >= 0, hi - lo, -1)
    bb, nbb = _blocks(n, J, BUCKET)
    out["max_bucket_entries"] = int(np.bincount(bb, minlength=nbb).max())
    return out


# ------------------------------------------------------------------------------------------------------------------ ragged
_RAGGED_P = np.array([0.05] + [0.03] * 11 + [0.62])   # run lengths 0 .. 12: many 12s, some 0s, mean 9.4


def _ragged_lengths(n, rng, head_empty=False, tail_empty=False):
    """run lengths 0 .. 12 with empty stretches of 256 (the first half of one pair, the second half of another), 512 (a pair),
    1024 (two pairs) and 300 columns (unaligned, across a bucket boundary), and one pair filled to the brim"""
    L = rng.choice(13, size=n, p=_RAGGED_P).astype(np.int64)
    npairs = n // PAIR
    assert npairs >= 16, "the stretches need 16 whole pairs"
    p = [int(npairs * f) for f in (0.1, 0.25, 0.4, 0.55, 0.7, 0.85)]
    marks = {}
    L[PAIR * p[0]: PAIR * p[0] + BUCKET] = 0                   # split == 0
    L[PAIR * p[1] + BUCKET: PAIR * p[1] + PAIR] = 0            # split == n
    L[PAIR * p[2]: PAIR * p[2] + PAIR] = 0                     # n == 0
    L[PAIR * p[3]: PAIR * p[3] + 2 * PAIR] = 0
    L[PAIR * p[4] + 100: PAIR * p[4] + 400] = 0
    L[PAIR * p[5]: PAIR * p[5] + PAIR] = RUN                   # 6144 entries: the pair kernel's capacity
    marks.update(empty_first_half=p[0], empty_second_half=p[1], empty_pairs=[p[2], p[3], p[3] + 1], unaligned=(PAIR * p[4] + 100, PAIR * p[4] + 400),
                 full_pair=p[5])
    if head_empty:
        L[:PAIR] = 0                                           # (the first pair: nothing in front of it to re-read)
        marks["empty_pairs"] = [0] + marks["empty_pairs"]
    if tail_empty:
        last = PAIR * ((n - 1) // PAIR)
        L[last:] = 0
        marks["empty_pairs"] = marks["empty_pairs"] + [(n - 1) // PAIR]
    return L, marks


def _near_rows(J, rng, m, lo=-3, hi=3, shift=0):
    return np.clip(J + shift + rng.integers(lo, hi + 1, len(J)), 1, m)


def _values(rng, count, zeros=0.10, negzeros=0.01):
    V = rng.standard_normal(count)
    u = rng.random(count)
    V[u < zeros] = 0.0
    V[(u >= zeros) & (u < zeros + negzeros)] = -0.0
    return V


RAGGED_MODS = (0, 1, 255, 256, 257)


def ragged(nmod=0, kind=UPDATE, seed=1, n_base=119808):
    """Run lengths 0 .. 12 (rows within +-3 of the diagonal: up to seven positions share a column's up to 12 updates, 10 % of the
    values 0.0, 1 % -0.0) with the empty stretches of _ragged_lengths.  n = n_base + nmod with n_base a multiple of 512: the last
    pair holds two full buckets (0), one column (1), a partial bucket (255), one bucket (256) or a bucket and one column (257).
    nmod 256 also empties the FIRST pair, nmod 257 the last."""
    assert n_base % PAIR == 0 and nmod in RAGGED_MODS
    n = n_base + nmod
    rng = np.random.default_rng([seed, nmod, 11])
    L, marks = _ragged_lengths(n, rng, head_empty=nmod == 256, tail_empty=nmod == 257)
    J, _ = _expand(L)
    I = _near_rows(J, rng, n)
    V = _values(rng, len(J))
    props = dict(marks, maxrun=RUN, last_pair_columns=n - PAIR * ((n - 1) // PAIR), density_window=(7.2, 12.0))
    return Stream(n, n, kind, I, J, V), props


def long_run(where, kind=UPDATE, seed=2, n_base=119808):
    """`ragged` with exactly ONE column of 13 entries, in a bucket that stays below 3072 entries (so that the host still chooses the
    pair kernel and the kernel's own run check is what refuses): where = "first_pair", "interior_second" (the second bucket of an
    interior pair) or "odd_last" (the lone bucket of the last pair; n = n_base + 255)."""
    nmod = 255 if where == "odd_last" else 0
    n = n_base + nmod
    rng = np.random.default_rng([seed, nmod, 13])
    L, marks = _ragged_lengths(n, rng)
    npairs = (n + PAIR - 1) // PAIR
    if where == "first_pair":
        c = 7
    elif where == "interior_second":
        c = PAIR * int(npairs * 0.47) + BUCKET + 77
    elif where == "odd_last":
        c = PAIR * (npairs - 1) + 100
    else:
        raise ValueError(where)
    L[c + 1: c + 17] = 4
    L[c] = RUN + 1
    J, _ = _expand(L)
    I = _near_rows(J, rng, n)
    V = _values(rng, len(J))
    props = dict(marks, maxrun=RUN + 1, long_column=c + 1, long_pair=c // PAIR, long_bucket=c // BUCKET)
    return Stream(n, n, kind, I, J, V), props


# --------------------------------------------------------------------------------------------------------- order_sensitive
BIG = 2.0 ** 60
TINY = 2.0 ** -60
SUBNORMAL = 5e-324
ZERO_PATTERNS = ("all_zero", "zero_first", "cancel", "neg_zero")


def _zero_pattern(name, k, copy):
    if name == "all_zero":
        return [0.0] * k
    if name == "zero_first":
        return [0.0] + [(1.0, TINY, -BIG, 3.0 * SUBNORMAL)[(i + copy) % 4] for i in range(k - 1)]
    if name == "cancel":                         # every partial sum is exact: x, 0, x, 0 ... and 1, 2, 0
        if k == 1:
            return [0.0]
        head = [1.0, 1.0, -2.0] if k % 2 else []
        return head + [x for i in range((k - len(head)) // 2) for x in ((BIG, -BIG) if (i + copy) % 2 == 0 else (-TINY, TINY))]
    if name == "neg_zero":
        return [-0.0] * k if copy % 2 == 0 else [-0.0] + [0.0] * (k - 1)
    raise ValueError(name)


def order_sensitive(kind=UPDATE, seed=3, n=120000):
    """Every column holds position A (row j + 8) with 3 .. 12 updates, often a position B (row j + 10) with 3 or more, and single
    updates of other rows on both sides of them, all in a random order inside the column: the sort has to bring the duplicates
    of a row together AND keep their append order.  The updates of A and B hold one +2^60 and one -2^60 among terms drawn from
    {1, 2^-60, subnormals} (a quarter of the columns: every term drawn from {2^60, -2^60, 1, 2^-60, subnormal}), so the sum depends
    on the order of its terms.  Chosen columns carry the zero patterns at every number of updates 1 .. 12 of position A: all 0.0;
    0.0 first, then non-zero terms; non-zero terms that cancel to exactly 0.0; -0.0.
    No NaN and no +-Inf anywhere: the sign and payload of a default NaN differ between the CPU and the GPU, and that is not what
    these streams test (no partial sum overflows either: at most 12 terms of magnitude 2^60)."""
    rng = np.random.default_rng([seed, 17])
    m = n + 16
    kA = rng.integers(3, 13, n)
    ncopies = max(1, n // 25000)
    nspecial = len(ZERO_PATTERNS) * 12 * ncopies
    stride = n // (nspecial + 2)
    assert stride >= 2
    special = {}
    for s in range(nspecial):
        c = (s + 1) * stride
        k, t, copy = s % 12 + 1, (s // 12) % len(ZERO_PATTERNS), s // (12 * len(ZERO_PATTERNS))
        special[c] = (k, ZERO_PATTERNS[t], copy)
        kA[c] = k
    Lraw = np.where(rng.random(n) < 0.75, 12, rng.integers(1, 13, n))
    L = np.maximum(kA, Lraw)
    rest = L - kA
    kB = np.where((rest >= 3) & (rng.random(n) < 0.6), 3 + (rng.random(n) * (rest - 2)).astype(np.int64), 0)
    kB = np.minimum(kB, rest)
    idx = np.arange(12)[None, :]
    isA = idx < kA[:, None]
    isB = (idx >= kA[:, None]) & (idx < (kA + kB)[:, None])
    isS = (idx >= (kA + kB)[:, None]) & (idx < L[:, None])
    pool = np.array([-6, -5, -4, -3, -2, -1, 1, 3, 4, 5, 6, 7], np.int64)       # rows of the single updates (A: 0, B: 2)
    pick = np.argsort(rng.random((n, 12)), axis=1)
    single_no = np.clip(idx - (kA + kB)[:, None], 0, 11)
    off = np.where(isA, 0, np.where(isB, 2, pool[np.take_along_axis(pick, single_no, axis=1)]))

    def smalls(shape):
        c = rng.integers(0, 3, shape)
        return np.where(c == 0, 1.0, np.where(c == 1, TINY, SUBNORMAL * rng.integers(1, 1000, shape)))

    def group_values(k):
        """n x 12: the terms of a group of k updates in APPEND order (columns >= k unused)"""
        G = smalls((n, 12))
        kk = np.maximum(k - 1, 2)        # (the last term is a small one: it survives in append order, in no other)
        pa = (rng.random(n) * kk).astype(np.int64)
        pb = (pa + 1 + (rng.random(n) * (kk - 1)).astype(np.int64)) % kk
        rows = np.arange(n)
        G[rows, pa] = BIG
        G[rows, pb] = -BIG
        free = rng.random(n) < 0.25
        c = rng.integers(0, 5, (n, 12))
        F = np.choose(c, [BIG, -BIG, 1.0, TINY, SUBNORMAL * 3.0])
        G[free] = F[free]
        return G

    GA, GB = group_values(kA), group_values(kB)
    for c, (k, name, copy) in special.items():
        GA[c, :k] = _zero_pattern(name, k, copy)
    c5 = rng.integers(0, 5, (n, 12))
    GS = np.where(c5 == 0, BIG, np.where(c5 == 1, -BIG, smalls((n, 12))))
    # the entries of a column in a random order; a group's terms keep their append order (the i-th A entry gets GA[:, i])
    perm = np.argsort(rng.random((n, 12)), axis=1)
    isA, isB, isS, off = (np.take_along_axis(x, perm, axis=1) for x in (isA, isB, isS, off))
    rankA = np.clip(np.cumsum(isA, axis=1) - 1, 0, 11)
    rankB = np.clip(np.cumsum(isB, axis=1) - 1, 0, 11)
    Vm = np.where(isA, np.take_along_axis(GA, rankA, axis=1), np.where(isB, np.take_along_axis(GB, rankB, axis=1), GS))
    used = isA | isB | isS
    col = np.broadcast_to(np.arange(1, n + 1, dtype=np.int64)[:, None], (n, 12))
    J = col[used]
    I = J + 8 + off[used]
    V = np.ascontiguousarray(Vm[used])
    assert np.all(np.isfinite(V)) and I.min() >= 1 and I.max() <= m
    props = dict(maxrun=RUN, special={c + 1: v for c, v in special.items()}, row_A=8, row_B=10, density_window=(7.2, 12.0))
    return Stream(m, n, kind, np.ascontiguousarray(I), np.ascontiguousarray(J), V), props


# -------------------------------------------------------------------------------------------------------------------- span
SPAN_SERVED = ((1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 19) - 1)
_FAR_PATTERN = ("r0", "far", 5, "far", "r0", "mid", "far", 3, "mid", "r0", "far", 1)    # a column of 12: duplicates interleaved


def span(variant="served", kind=UPDATE, seed=4, n=150000):
    """m = 2^21; rows j .. j + 6 in every column, 8 .. 12 updates per column (no zero values), except in chosen pairs:
      "served":      four pairs whose FIRST column also holds rows r0 + d (r0 its diagonal row, the pair's smallest) for d = 2^18 - 1,
                     2^18, 2^18 + 1 and 2^19 - 1 -- the pair's row span is exactly d, and from 2^18 on bit 31 of the sort key differs
                     inside one column (12 updates of the rows r0, r0 + 1 .. 5, r0 + 2^17 and r0 + d, duplicates interleaved);
      "refused":     one pair of that shape with d = 2^19, nothing else far from the diagonal;
      "two_columns": two pairs with d = 2^18 and 2^19 - 1 where r0 lies in the pair's first bucket and r0 + d in a column of its second."""
    rng = np.random.default_rng([seed, 19])
    m = 1 << 21
    L = rng.integers(8, 13, n).astype(np.int64)
    npairs = n // PAIR
    if variant == "served":
        chosen = {int(npairs * f): d for f, d in zip((0.07, 0.31, 0.55, 0.79), SPAN_SERVED)}
    elif variant == "refused":
        chosen = {int(npairs * 0.43): ROW_SPAN}
    elif variant == "two_columns":
        chosen = {int(npairs * 0.23): 1 << 18, int(npairs * 0.67): ROW_SPAN - 1}
    else:
        raise ValueError(variant)
    far_col = {p: PAIR * p + (300 if variant == "two_columns" else 0) for p in chosen}     # 0-based
    for p in chosen:
        L[PAIR * p] = RUN
        L[far_col[p]] = RUN
    L[PAIR * (npairs // 2 + 3): PAIR * (npairs // 2 + 4)] = RUN      # (a pair filled to the brim: see the module docstring)
    J, q = _expand(L)
    I = J + rng.integers(0, 7, len(J))
    V = rng.standard_normal(len(J))
    V[V == 0.0] = 1.0
    start = np.cumsum(L) - L
    for p, d in chosen.items():
        r0 = PAIR * p + 1
        I[start[PAIR * p]] = r0                                     # the pair's smallest row: its first column's diagonal
        base = {"r0": r0, "far": r0 + d, "mid": r0 + (1 << 17)}
        c = far_col[p]
        rows = [base[x] if isinstance(x, str) else r0 + (c - PAIR * p) + x for x in _FAR_PATTERN]
        if variant == "two_columns":
            rows = [r for r in rows if r != r0] + [r0 + 300] * 3
        I[start[c]: start[c] + RUN] = rows[:RUN]
    assert I.max() <= m
    props = dict(maxrun=RUN, spans=chosen, far_columns={p: c + 1 for p, c in far_col.items()}, density_window=(7.2, 12.0))
    return Stream(m, n, kind, I, J, V), props


# ------------------------------------------------------------------------------------------------------------------ repeat
def _repeat_base(n, rng, m=None):
    """the common shape of the repeat_* sequences: ragged run lengths without the long empty stretches, rows j + 5 .. j + 11,
    one pair filled to the brim; a fixed mask of zero values"""
    m = n + 16 if m is None else m
    L = rng.choice(13, size=n, p=_RAGGED_P).astype(np.int64)
    npairs = n // PAIR
    L[PAIR * (npairs // 3): PAIR * (npairs // 3 + 1)] = RUN
    return m, L


def _batch_values(seed, k, count, zero_mask):
    V = np.random.default_rng([seed, 23, k]).standard_normal(count)
    V[V == 0.0] = 1.0
    V[zero_mask] = 0.0
    return V


def repeat_a(kind=UPDATE, seed=5, n=140000, batches=3):
    """(a) the same rows, columns and zero values in every batch; new non-zero values"""
    rng = np.random.default_rng([seed, 29])
    m, L = _repeat_base(n, rng)
    J, _ = _expand(L)
    I = _near_rows(J, rng, m, shift=8)
    Z = rng.random(len(J)) < 0.10
    out = [(I, J, _batch_values(seed, k, len(J), Z)) for k in range(batches)]
    return m, n, kind, out, dict(maxrun=RUN, states=[0] + [1] * (batches - 1))


def repeat_b(kind=UPDATE, seed=6, n=140000, batches=3):
    """(b) batch k holds the rows of batch 0 moved down by k: other positions, the same number of created positions in every
    column (the zero values stay where they are)"""
    rng = np.random.default_rng([seed, 31])
    m, L = _repeat_base(n, rng)
    J, _ = _expand(L)
    I = _near_rows(J, rng, m - 4, shift=8)
    Z = rng.random(len(J)) < 0.10
    out = [(I + k, J, _batch_values(seed, k, len(J), Z)) for k in range(batches)]
    return m, n, kind, out, dict(maxrun=RUN, states=[0] + [1] * (batches - 1))


def _swap_sequence(seed, n, gap_pairs, tag):
    """kind UPDATE: columns a and b each hold one position (row j + 8 + 6, outside the other rows of the column) with two updates.
    Batch 0: a's two are non-zero, b's both 0.0 (never created); batches 1 and 2: a's both 0.0, b's non-zero."""
    rng = np.random.default_rng([seed, tag])
    m, L = _repeat_base(n, rng)
    P = int((n // PAIR) * 0.6)
    a, b = PAIR * P + 10, PAIR * (P + gap_pairs) + (400 if gap_pairs == 0 else 20)      # 0-based columns
    L[a] = L[b] = 10
    J, q = _expand(L)
    I = _near_rows(J, rng, m, shift=8)
    Z = rng.random(len(J)) < 0.10
    start = np.cumsum(L) - L
    ea, eb = np.array([start[a] + 2, start[a] + 7]), np.array([start[b] + 1, start[b] + 6])
    I[ea] = a + 1 + 8 + 6
    I[eb] = b + 1 + 8 + 6
    Z[ea] = Z[eb] = False
    out = []
    for k in range(3):
        V = _batch_values(seed, k, len(J), Z)
        V[ea if k else eb] = 0.0
        out.append((I, J, V))
    return m, out, dict(maxrun=RUN, a=a + 1, b=b + 1, pair_a=a // PAIR, pair_b=b // PAIR)


def repeat_c(seed=7, n=140000):
    """(c) a position of column a goes to all-zero while one of column b in the SAME pair becomes non-zero: every pair emits what
    the table says, the flush is served -- and the colptr between a and b moves by one"""
    m, out, props = _swap_sequence(seed, n, 0, 37)
    return m, n, UPDATE, out, dict(props, states=[0, 1, 1])


def repeat_d(seed=8, n=140000):
    """(d) the same with a and b in NEIGHBOURING pairs: two pairs emit another count -- missed, then (batch 2 has the shape of
    batch 1) served from the table the miss left"""
    m, out, props = _swap_sequence(seed, n, 1, 41)
    return m, n, UPDATE, out, dict(props, states=[0, 2, 1])


def repeat_e(kind=UPDATE, seed=9, n=140000):
    """(e) m = 2^21; batch 1 moves one update of one pair 2^19 + 600 rows down (no other update shares its position before or
    after: the counts stay): that pair now spans 2^19 or more and is refused; batch 2 is batch 0 with new values"""
    rng = np.random.default_rng([seed, 43])
    m, L = _repeat_base(n, rng, m=1 << 21)
    P = int((n // PAIR) * 0.45)
    c = PAIR * P + 130
    L[c] = 10
    J, _ = _expand(L)
    I = _near_rows(J, rng, m, shift=8)
    Z = rng.random(len(J)) < 0.10
    e = (np.cumsum(L) - L)[c] + 4
    I[e] = c + 1 + 8 + 6
    Z[e] = False
    I1 = I.copy()
    I1[e] += ROW_SPAN + 600
    out = [(I, J, _batch_values(seed, 0, len(J), Z)), (I1, J, _batch_values(seed, 1, len(J), Z)), (I, J, _batch_values(seed, 2, len(J), Z))]
    return m, n, kind, out, dict(maxrun=RUN, moved_pair=P, states=[0, 2, 0], pairs=[1, 0, 0])


def repeat_g(where, kind=UPDATE, seed=11, n=140000):
    """(g) batches 0 and 1 as in (a), but in batch 1 one column of 12 entries holds a 13th, taken from a later column of the SAME
    bucket: every position of the stream lies in the bucket it lay in, so the producer's plan is batch 0's and the flush is tried
    in the predicted form -- which refuses for the run length; batch 2 is batch 0 with new values.  where = "first_pair" or
    "odd_last" (the lone bucket of the last pair: n mod 512 is between 1 and 256)"""
    rng = np.random.default_rng([seed, 59])
    m, L = _repeat_base(n, rng)
    lo = {"first_pair": 0, "odd_last": PAIR * ((n - 1) // PAIR)}[where]
    hi = min(lo + BUCKET, n)
    assert where == "first_pair" or n - lo <= BUCKET
    c = lo + 7 + int(np.flatnonzero(L[lo + 7:hi] == RUN)[0])      # the column that grows
    d = c + 1 + int(np.flatnonzero(L[c + 1:hi] >= 2)[0])          # the column that gives an entry (and keeps one)
    L1 = L.copy()
    L1[c] += 1
    L1[d] -= 1
    J, _ = _expand(L)
    J1, _ = _expand(L1)
    I = _near_rows(J, rng, m, shift=8)
    I1 = I + (J1 - J)                                             # (an entry that changes its column keeps its distance from the diagonal)
    assert I1.min() >= 1
    Z = rng.random(len(J)) < 0.10
    out = [(I, J, _batch_values(seed, 0, len(J), Z)), (I1, J1, _batch_values(seed, 1, len(J), Z)), (I, J, _batch_values(seed, 2, len(J), Z))]
    return m, n, kind, out, dict(maxrun=RUN + 1, long_column=c + 1, donor_column=d + 1, long_pair=c // PAIR, states=[0, 2, 0], pairs=[1, 0, 0])


def repeat_f(seed=10, n=140000, batches=4):
    """(f) kind UPDATE, 10 % zero values drawn anew in every batch: positions whose updates are all 0.0 are not created, so every
    batch emits other counts than the one before in thousands of pairs"""
    rng = np.random.default_rng([seed, 47])
    m, L = _repeat_base(n, rng)
    J, _ = _expand(L)
    I = _near_rows(J, rng, m, shift=8)
    out = []
    for k in range(batches):
        Z = np.random.default_rng([seed, 53, k]).random(len(J)) < 0.10
        out.append((I, J, _batch_values(seed, k, len(J), Z)))
    return m, n, UPDATE, out, dict(maxrun=RUN, states=[0, 2, 2, 0][:batches])
