"""CPU: the streams of tests/pair_streams.py have the properties tests/test_pair_oracle_gpu.py relies on -- checked with numpy and the
oracle, so that a GPU test cannot pass for the wrong reason -- and the oracle agrees with the dict model (tests/refmodel.py) on a
scaled-down copy of every builder."""
import numpy as np
import pytest

import pair_streams as ps
from refmodel import COO as MODEL_COO, DictModel, assert_csc_equal, bits

SMALL = 16 * ps.PAIR       # columns of a scaled-down copy: the fewest the stretches of `ragged` fit into


def _check_window(s):
    """what the host asks before it chooses the pair kernel, as far as a stream decides it"""
    assert s.I.dtype == np.int64 and s.J.dtype == np.int64 and s.V.dtype == np.float64
    assert len(s.I) == len(s.J) == len(s.V)
    assert np.all(np.diff(s.J) >= 0), "J ascending"
    assert s.I.min() >= 1 and s.I.max() <= s.m and s.J.min() >= 1 and s.J.max() <= s.n
    assert 100000 <= s.n <= 300000
    assert 4096 < len(s.J) <= 12 * s.n
    d = len(s.J) / s.n
    assert 7.2 < d <= 12.0, d                                   # 256-column buckets (pair_streams' docstring)
    assert s.m < 2 ** 31                                        # fewer than 32 row bits
    assert np.all(np.isfinite(s.V))


def _block_nnz(colptr, n, width=ps.PAIR):
    edges = np.minimum(np.arange(0, n + width, width), n)
    return np.diff(colptr[edges])


@pytest.mark.parametrize("nmod", ps.RAGGED_MODS)
def test_ragged(nmod):
    s, p = ps.ragged(nmod)
    _check_window(s)
    assert s.n % ps.PAIR == nmod
    d = ps.describe(s.m, s.n, s.I, s.J)
    runs = np.bincount(s.J - 1, minlength=s.n)
    assert d["maxrun"] == 12 and set(np.unique(runs).tolist()) == set(range(13)), "every run length 0 .. 12"
    assert (runs == 12).mean() > 0.5 and (runs == 0).mean() > 0.04
    assert d["max_bucket_entries"] == ps.BUCKET_ENTRIES         # a bucket filled to the brim: the cut stays at 256 columns
    assert runs[ps.PAIR * p["full_pair"]: ps.PAIR * (p["full_pair"] + 1)].sum() == 6144
    assert d["empty_pairs"] == sorted(p["empty_pairs"])
    nbuckets = (s.n + ps.BUCKET - 1) // ps.BUCKET
    want = {2 * p["empty_first_half"], 2 * p["empty_second_half"] + 1}
    for q in p["empty_pairs"]:
        want |= {b for b in (2 * q, 2 * q + 1) if b < nbuckets}
    assert set(d["empty_buckets"]) == want
    lo, hi = p["unaligned"]
    assert lo % ps.BUCKET and hi % ps.BUCKET and lo // ps.BUCKET != hi // ps.BUCKET
    assert runs[lo:hi].sum() == 0 and runs[lo - 20:lo].sum() > 0 and runs[hi:hi + 20].sum() > 0
    assert p["last_pair_columns"] == {0: 512, 1: 1, 255: 255, 256: 256, 257: 257}[nmod]
    assert (0 in d["empty_pairs"]) == (nmod == 256) and ((s.n - 1) // ps.PAIR in d["empty_pairs"]) == (nmod == 257)
    assert d["pair_span"].max() < 1024                          # (bit 31 of the sort key never set: `span` is the stream for that)
    # positions with three or more updates: a fold that permutes equal rows changes bits here as well
    key = s.J * (s.m + 1) + s.I
    _, cnt = np.unique(key, return_counts=True)
    assert (cnt >= 3).sum() > 50000


@pytest.mark.parametrize("where", ["first_pair", "interior_second", "odd_last"])
def test_long_run(where):
    s, p = ps.long_run(where)
    _check_window(s)
    runs = np.bincount(s.J - 1, minlength=s.n)
    assert runs.max() == 13 and (runs == 13).sum() == 1 and int(np.argmax(runs)) + 1 == p["long_column"]
    c = p["long_column"] - 1
    per_bucket = np.bincount((s.J - 1) // ps.BUCKET)
    assert per_bucket.max() <= ps.BUCKET_ENTRIES                # the host's condition holds: the KERNEL meets the run of 13
    assert per_bucket[c // ps.BUCKET] <= ps.BUCKET_ENTRIES - 40
    npairs = (s.n + ps.PAIR - 1) // ps.PAIR
    if where == "first_pair":
        assert c // ps.PAIR == 0
    elif where == "interior_second":
        assert 0 < c // ps.PAIR < npairs - 1 and (c // ps.BUCKET) % 2 == 1
    else:
        assert c // ps.PAIR == npairs - 1 and s.n - ps.PAIR * (npairs - 1) <= ps.BUCKET
    assert ps.describe(s.m, s.n, s.I, s.J)["pair_span"].max() < 1024


@pytest.mark.parametrize("variant", ["served", "refused", "two_columns"])
def test_span(variant):
    s, p = ps.span(variant)
    _check_window(s)
    assert s.m >= 2 ** 21
    d = ps.describe(s.m, s.n, s.I, s.J)
    assert d["maxrun"] == 12 and d["max_bucket_entries"] == ps.BUCKET_ENTRIES
    sp = d["pair_span"]
    for q, want in p["spans"].items():
        assert sp[q] == want, (q, sp[q], want)                  # exactly
    others = np.delete(sp, list(p["spans"]))
    assert others.max() < 1024
    want = {"served": [2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 19 - 1], "refused": [2 ** 19], "two_columns": [2 ** 18, 2 ** 19 - 1]}[variant]
    assert sorted(p["spans"].values()) == want
    assert (sp >= ps.ROW_SPAN).sum() == (1 if variant == "refused" else 0)
    for q, dd in p["spans"].items():
        r0 = ps.PAIR * q + 1
        first = s.I[s.J == r0]
        far = s.I[s.J == p["far_columns"][q]]
        assert first.min() == r0 and far.max() == r0 + dd
        if variant == "two_columns":
            assert (p["far_columns"][q] - 1) // ps.BUCKET == 2 * q + 1 and first.max() < r0 + 1024 and far.min() > r0
        else:
            # bit 31 of (row - rmin) << 13 differs INSIDE the column, and its duplicates are interleaved with other rows
            assert p["far_columns"][q] == r0 and far.min() == r0
            k = ((far - r0).astype(np.uint64) << np.uint64(13)) & np.uint64(0xFFFFFFFF)
            assert ((k >> np.uint64(31)).max() == 1) == (2 ** 18 <= dd < 2 ** 19)
            assert (far == r0 + dd).sum() >= 3 and np.diff(np.flatnonzero(far == r0 + dd)).min() > 1
        assert np.all(s.V[s.J == p["far_columns"][q]] != 0.0)


def _ordered_sum(M, valid):
    acc = np.zeros(len(M))
    for t in range(M.shape[1]):
        acc = np.where(valid[:, t], acc + M[:, t], acc)
    return acc


def test_order_sensitive(orc):
    s, p = ps.order_sensitive(kind=ps.RAWUPDATE)
    _check_window(s)
    assert not np.any(np.isnan(s.V)) and not np.any(np.isinf(s.V))
    runs = np.bincount(s.J - 1, minlength=s.n)
    assert runs.max() == 12
    # the updates of every position in append order, as a padded matrix
    key = s.J * (s.m + 1) + s.I
    o = np.argsort(key, kind="stable")
    ks = key[o]
    head = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cnt = np.diff(np.r_[head, len(ks)])
    rank = np.arange(len(ks)) - np.repeat(head, cnt)
    M = np.zeros((len(head), 12))
    valid = np.zeros((len(head), 12), bool)
    pos = np.repeat(np.arange(len(head)), cnt)
    M[pos, rank] = s.V[o]
    valid[pos, rank] = True
    cp, rv, nz = ps.oracle_csc(orc, *s)
    assert len(nz) == len(head)                                 # RAWUPDATE: every position is created
    fwd = _ordered_sum(M, valid)
    assert np.array_equal(bits(fwd), bits(nz)), "the oracle sums in append order"
    multi = cnt >= 3
    assert multi.sum() >= s.n and cnt[multi].max() == 12 and set(np.unique(cnt[multi]).tolist()) == set(range(3, 13))
    # (a two-term sum is commutative: no such position but the zero patterns with two updates)
    assert (cnt == 2).sum() == sum(1 for k, _, _ in p["special"].values() if k == 2)
    # reversed order
    Mr = np.zeros_like(M)
    Mr[pos, cnt[pos] - 1 - rank] = s.V[o]
    rev = _ordered_sum(Mr, valid)
    # ascending by value
    Ms = np.where(valid, M, np.inf)
    Ms.sort(axis=1)
    srt = _ordered_sum(np.where(valid, Ms, 0.0), valid)
    for name, other in (("reversed", rev), ("sorted", srt)):
        frac = (bits(other)[multi] != bits(nz)[multi]).mean()
        print("order_sensitive:", name, "order changes %.3f of the %d positions with three or more updates" % (frac, multi.sum()))
        assert frac >= 0.5, (name, frac)
    # the duplicates of a position are interleaved with other rows of the column
    first_e = np.full(len(head), len(ks))
    last_e = np.zeros(len(head), np.int64)
    np.minimum.at(first_e, pos, o)
    np.maximum.at(last_e, pos, o)
    assert ((last_e - first_e + 1 > cnt)[multi]).mean() >= 0.5
    # the zero patterns, at every number of updates 1 .. 12
    seen = set()
    for col, (k, name, copy) in p["special"].items():
        got = s.V[(s.J == col) & (s.I == col + p["row_A"])]
        want = np.array(ps._zero_pattern(name, k, copy))
        assert len(got) == k and np.array_equal(bits(got), bits(want)), (col, k, name)
        seen.add((k, name))
        if name == "cancel" and k > 1:
            assert np.all(want != 0.0) and _ordered_sum(want[None, :], np.ones((1, k), bool))[0] == 0.0
        if name == "zero_first" and k > 1:
            assert want[0] == 0.0 and np.all(want[1:] != 0.0)
    assert seen == {(k, name) for k in range(1, 13) for name in ps.ZERO_PATTERNS}
    # under UPDATE the all-zero and -0.0 positions are not created, the cancelling ones are kept as 0.0
    cpu, rvu, nzu = ps.oracle_csc(orc, s.m, s.n, ps.UPDATE, s.I, s.J, s.V)
    for col, (k, name, copy) in p["special"].items():
        rows = rvu[cpu[col - 1] - 1: cpu[col] - 1]
        there = (col + p["row_A"]) in rows
        assert there == (name in ("zero_first", "cancel") and k > 1), (col, k, name)
        if there and name == "cancel":
            assert nzu[cpu[col - 1] - 1 + int(np.flatnonzero(rows == col + p["row_A"])[0])] == 0.0


def _oracle_batches(orc, m, n, kind, batches):
    return [ps.oracle_csc(orc, m, n, kind, *b) for b in batches]


def test_repeat_a_and_b(orc):
    for build in (ps.repeat_a, ps.repeat_b):
        m, n, kind, batches, p = build()
        for b in batches:
            _check_window(ps.Stream(m, n, kind, *b))
            assert np.array_equal(b[1], batches[0][1])
            assert np.array_equal(b[2] == 0.0, batches[0][2] == 0.0)
        assert not np.array_equal(batches[0][2], batches[1][2])
        got = _oracle_batches(orc, m, n, kind, batches)
        per = [_block_nnz(cp, n) for cp, _, _ in got]
        assert all(np.array_equal(per[0], x) for x in per[1:])          # what the predicted form validates
        assert all(np.array_equal(got[0][0], x[0]) for x in got[1:])
        if build is ps.repeat_a:
            assert all(np.array_equal(b[0], batches[0][0]) for b in batches)
            assert np.array_equal(got[0][1], got[1][1])
        else:
            assert np.array_equal(batches[1][0], batches[0][0] + 1)
            assert not np.array_equal(got[0][1], got[1][1])             # other rows
        assert p["states"] == [0, 1, 1]


def test_repeat_c_and_d(orc):
    for build in (ps.repeat_c, ps.repeat_d):
        m, n, kind, batches, p = build()
        assert kind == ps.UPDATE
        for b in batches:
            _check_window(ps.Stream(m, n, kind, *b))
            assert np.array_equal(b[0], batches[0][0]) and np.array_equal(b[1], batches[0][1])
        got = _oracle_batches(orc, m, n, kind, batches)
        per = [_block_nnz(cp, n) for cp, _, _ in got]
        a, b = p["a"], p["b"]
        assert a < b
        d01 = got[1][0] - got[0][0]
        # column a lost a position, column b gained one: colptr[a + 1 .. b] (1-based columns) moved by one, nothing else
        want = np.zeros(n + 1, np.int64)
        want[a:b] = -1
        assert np.array_equal(d01, want)
        assert np.array_equal(got[1][0], got[2][0])
        if build is ps.repeat_c:
            assert p["pair_a"] == p["pair_b"] and (a - 1) // ps.BUCKET != (b - 1) // ps.BUCKET
            assert np.array_equal(per[0], per[1]) and np.array_equal(per[1], per[2])
        else:
            assert p["pair_b"] == p["pair_a"] + 1
            diff = np.flatnonzero(per[0] != per[1])
            assert diff.tolist() == [p["pair_a"], p["pair_b"]]
            assert (per[1] - per[0])[diff].tolist() == [-1, 1]
            assert np.array_equal(per[1], per[2])


def test_repeat_e_and_f(orc):
    m, n, kind, batches, p = ps.repeat_e()
    assert m >= 2 ** 21
    for b in batches:
        _check_window(ps.Stream(m, n, kind, *b))
    spans = [ps.describe(m, n, b[0], b[1])["pair_span"] for b in batches]
    assert spans[0].max() < 1024 and spans[2].max() < 1024
    assert (spans[1] >= ps.ROW_SPAN).sum() == 1 and spans[1][p["moved_pair"]] >= ps.ROW_SPAN
    got = _oracle_batches(orc, m, n, kind, batches)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], got[2][0])      # the counts stay
    m, n, kind, batches, p = ps.repeat_f()
    assert kind == ps.UPDATE and len(batches) == 4
    got = _oracle_batches(orc, m, n, kind, batches)
    per = [_block_nnz(cp, n) for cp, _, _ in got]
    for x, y in zip(per, per[1:]):
        assert (x != y).mean() > 0.5


@pytest.mark.parametrize("where", ["first_pair", "odd_last"])
def test_repeat_g(where):
    m, n, kind, batches, p = ps.repeat_g(where)
    for b in batches:
        _check_window(ps.Stream(m, n, kind, *b))
    (I0, J0, V0), (I1, J1, V1), (I2, J2, V2) = batches
    assert np.array_equal(I2, I0) and np.array_equal(J2, J0) and not np.array_equal(V2, V0)
    assert np.array_equal(V1 == 0.0, V0 == 0.0) and np.array_equal(V2 == 0.0, V0 == 0.0)
    # the producer's plan is batch 0's: every position of the stream lies in the bucket it lay in
    assert np.array_equal((J1 - 1) // ps.BUCKET, (J0 - 1) // ps.BUCKET)
    nb = (n + ps.BUCKET - 1) // ps.BUCKET
    per0, per1 = (np.bincount((J - 1) // ps.BUCKET, minlength=nb) for J in (J0, J1))
    assert np.array_equal(per1, per0) and per0.max() <= ps.BUCKET_ENTRIES
    # exactly one column has a run of 13, no run is longer, and it took its 13th entry from a column of its own bucket
    runs0, runs1 = (np.bincount(J - 1, minlength=n) for J in (J0, J1))
    c, d = p["long_column"] - 1, p["donor_column"] - 1
    assert runs0.max() == 12 and runs0[c] == 12
    assert runs1.max() == 13 and (runs1 == 13).sum() == 1 and int(np.argmax(runs1)) == c
    assert np.flatnonzero(runs1 != runs0).tolist() == [c, d] and runs1[d] == runs0[d] - 1 >= 1
    assert c // ps.BUCKET == d // ps.BUCKET
    npairs = (n + ps.PAIR - 1) // ps.PAIR
    if where == "first_pair":
        assert c // ps.PAIR == 0 == p["long_pair"]
    else:
        assert c // ps.PAIR == npairs - 1 == p["long_pair"] and 0 < n - ps.PAIR * (npairs - 1) <= ps.BUCKET
    # (nothing else the pair kernels refuse: the rows of every pair stay close)
    assert all(ps.describe(m, n, b[0], b[1])["pair_span"].max() < 1024 for b in batches)
    assert p["states"] == [0, 2, 0] and p["pairs"] == [1, 0, 0]


def _small_cases():
    nb = SMALL
    yield "ragged", ps.ragged(1, kind=ps.UPDATE, n_base=nb)[0]
    yield "ragged_set", ps.ragged(255, kind=ps.SET, n_base=nb)[0]
    yield "order_sensitive_update", ps.order_sensitive(kind=ps.UPDATE, n=nb + 100)[0]
    yield "order_sensitive_raw", ps.order_sensitive(kind=ps.RAWUPDATE, n=nb + 100)[0]
    yield "order_sensitive_set", ps.order_sensitive(kind=ps.SET, n=nb + 100)[0]
    yield "order_sensitive_coo", ps.order_sensitive(kind=ps.COO, n=nb + 100)[0]
    for v, kind in (("served", ps.UPDATE), ("refused", ps.RAWUPDATE), ("two_columns", ps.COO)):
        yield "span_" + v, ps.span(v, kind=kind, n=nb + 300)[0]
    for w, kind in (("first_pair", ps.UPDATE), ("interior_second", ps.SET), ("odd_last", ps.RAWUPDATE)):
        yield "long_run_" + w, ps.long_run(w, kind=kind, n_base=nb)[0]
    for name in "abcdef":
        m, n, kind, batches, _ = getattr(ps, "repeat_" + name)(n=nb + 77)
        for k in (0, 1):
            yield "repeat_%s_%d" % (name, k), ps.Stream(m, n, kind, *batches[k])
    for w, kind in (("first_pair", ps.UPDATE), ("odd_last", ps.RAWUPDATE)):
        m, n, kind, batches, _ = ps.repeat_g(w, kind=kind, n=nb + 77)
        yield "repeat_g_" + w, ps.Stream(m, n, kind, *batches[1])


def test_oracle_agrees_with_dict_model(orc):
    """a second, independent reference on a scaled-down copy of every builder (16 pairs), every kind, and op "-" on one of them"""
    count = 0
    for name, s in _small_cases():
        for sub in ((False, True) if name in ("order_sensitive_update", "ragged") else (False,)):
            M = DictModel(s.m, s.n)
            kind = MODEL_COO if s.kind == ps.COO else s.kind
            V = -s.V if (sub and s.kind != ps.SET) else s.V
            for i, j, v in zip(s.I.tolist(), s.J.tolist(), V.tolist()):
                M.apply(kind, v, i, j)
            assert_csc_equal(ps.oracle_csc(orc, *s, sub=sub), M.arrays(), name)
            count += 1
    assert count >= 24
