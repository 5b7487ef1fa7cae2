"""The pair bucket kernels (csrc/local_w.hip: pair_k, pair_pred_k, pair_record_k, built from the phase functions there and in
csrc/pair.hpp) against the CPU ORACLE at their edges.

tests/test_bucket_pairs_gpu.py and tests/test_predicted_offsets_gpu.py compare these kernels with their sibling local_k on two
stream shapes; here every flush -- on an automatic handle AND on one pinned to one bucket per workgroup (esp_debug_force_path 42) --
is compared bit for bit (colptr, rowval, nzval) with the oracle, on the streams of tests/pair_streams.py: ragged run lengths
0 .. 12 with empty buckets and pairs, sums whose bits depend on the order of their terms, pairs whose rows span up to 2^19 - 1
(bit 31 of the sort key) or 2^19 (refused), a column run of 13 (refused), buckets narrower than 256 columns, and repeated plans
whose rows, zeros, spans and run lengths move (the predicted form).  What ran is asserted with the esp_debug_last_* queries; a precondition
that does not hold fails the test.  tests/test_pair_streams.py checks on the CPU that the streams are what they claim to be."""
import collections

import numpy as np
import pytest

import pair_streams as ps
from refmodel import assert_csc_equal

pytestmark = pytest.mark.gpu

NO_PAIRS = 42
SEED_A, SEED_B = 0x5EED0002, 0x5EED0B0B
KINDS = (ps.SET, ps.UPDATE, ps.RAWUPDATE, ps.COO)

What = collections.namedtuple("What", "pairs predicted key_bytes small reused cl_bits buckets")


def _what(A):
    cl, nb = A.debug_last_bucket_cut()
    return What(A.debug_last_bucket_pairs(), A.debug_last_predicted(), A.debug_last_key_bytes(), A.debug_last_local_small(),
                A.debug_last_plan_reused(), cl, nb)


def _resident(*arrs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrs)


def _append(A, kind, I, J, V, how, op="+"):
    if how == "host":
        A.append(kind, I, J, V, op=op)
    elif how == "host_i32":
        A.append(kind, I.astype(np.int32), J.astype(np.int32), V, op=op)
    else:
        dev = _resident(I, J, V)
        A.append_device(kind, *dev, op=op)
        A._keep = dev      # (the arrays stay alive until the flush has read them)


def _matrix(esp, m, n, force=0, cap=0.0):
    A = esp.ExtendableSparseMatrix(m, n)
    A.debug_force_path(force)
    if cap:
        A.debug_plan_cap(cap)
    return A


_STREAMS = {}


def _stream(name):
    """(Stream of kind UPDATE, props) by name, built once"""
    if name not in _STREAMS:
        if name.startswith("ragged_"):
            _STREAMS[name] = ps.ragged(int(name.split("_")[1]))
        elif name == "order_sensitive":
            _STREAMS[name] = ps.order_sensitive()
        elif name.startswith("span_"):
            _STREAMS[name] = ps.span(name[5:])
        elif name.startswith("long_run_"):
            _STREAMS[name] = ps.long_run(name[9:])
        else:
            raise KeyError(name)
    return _STREAMS[name]


def _served_once(esp, orc, s, kind, how, op, label, want=None):
    """one stream on an automatic and on a pinned handle: both the oracle's bits; the automatic one through the pair kernel"""
    if want is None:
        want = ps.oracle_csc(orc, s.m, s.n, kind, s.I, s.J, s.V, sub=op == "-")
    seen = []
    for force in (0, NO_PAIRS):
        A = _matrix(esp, s.m, s.n, force)
        _append(A, kind, s.I, s.J, s.V, how, op)
        A.flush()
        w = _what(A)
        print(label, "kind", kind, how, op, "force", force, w, "nnz", len(want[1]))
        assert_csc_equal(A.arrays(), want, "%s kind %d %s %s force %d:" % (label, kind, how, op, force))
        assert w.key_bytes == 4 and w.small == 1 and w.cl_bits == 8, (label, kind, how, op, force, w)
        assert w.pairs == (1 if force == 0 else 0), (label, kind, how, op, force, w)
        assert w.predicted == 0, (label, w)
        assert w.buckets >= (s.n + ps.BUCKET - 1) // ps.BUCKET
        seen.append(w)
    return want, seen


SERVED = ["ragged_%d" % x for x in ps.RAGGED_MODS] + ["order_sensitive"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SERVED)
def test_served_kinds_ops_entry_points(esp, orc, name, kind):
    """ragged (every n mod 512) and order_sensitive x SET / UPDATE / RAWUPDATE / COO x "+" / "-" x esp_append_host / esp_append_device:
    pair_k<2> for UPDATE, pair_k<1> with the fold chosen by the kind at run time for the others"""
    s, _ = _stream(name)
    for op in ("+", "-"):
        want = None
        for how in ("host", "device"):
            want, _ = _served_once(esp, orc, s, kind, how, op, name, want)


@pytest.mark.parametrize("name", ["span_served", "span_two_columns"])
def test_served_row_spans(esp, orc, name):
    """pairs whose rows span exactly 2^18 - 1, 2^18, 2^18 + 1 and 2^19 - 1 (bit 31 of the sort key set from 2^18 on, inside one
    column or between the pair's two buckets): served, the oracle's bits"""
    s, p = _stream(name)
    assert max(p["spans"].values()) == ps.ROW_SPAN - 1
    for kind in (ps.UPDATE, ps.RAWUPDATE):
        for how in ("host", "device"):
            _served_once(esp, orc, s, kind, how, "+", name)


def test_served_int32_indices(esp, orc):
    """esp_append_host_i32 (Ti = Int32 arrays as they are) into the pair kernel"""
    s, _ = _stream("ragged_255")
    _served_once(esp, orc, s, ps.UPDATE, "host_i32", "+", "ragged_255 int32")


def _repeat_on_handle(esp, orc, A, m, n, kind, batches, label, how="device"):
    """the batches on ONE handle (reset! between them), each against the oracle; what every flush did"""
    out = []
    for i, (I, J, V) in enumerate(batches):
        A.reset()
        _append(A, kind, I, J, V, how)
        A.flush()
        w = _what(A)
        print(label, "kind", kind, "batch", i, w, "nnz", A.nnz())
        want = ps.oracle_csc(orc, m, n, kind, I, J, V)
        got = A.arrays()
        assert np.array_equal(got[0], want[0]), "%s batch %d: colptr differs (first at column %d)" % (
            label, i, int(np.flatnonzero(got[0] != want[0])[0]))
        assert_csc_equal(got, want, "%s batch %d:" % (label, i))
        out.append(w)
    return out


@pytest.mark.parametrize("cols", [128, 64, 32, 8])
@pytest.mark.parametrize("name", ["ragged_257", "order_sensitive"])
def test_narrow_buckets(esp, orc, name, cols):
    """esp_debug_plan_cap derived from the stream's density: buckets of 128, 64, 32 and 8 columns (cl_bits 7, 6, 5, 3: ncl < 512,
    idle lanes, other ncl_bits in pair_record_k) on the first flush; flushed again -- four times in all -- on the same handle
    after reset! so that pair_record_k and pair_pred_k run on narrow buckets too.  From its second flush on a handle plans with
    what the first one saw (plan_prefix_bits, seen_spread) and takes one prefix bit less where the fullest bucket still fits
    twice: buckets twice as wide (cl_bits 8, 7, 6, 4), a new plan -- the second flush records, the third and fourth are served.
    So the predicted form runs with cl_bits 7, 6 and 4; with 128 columns asked for it runs on full 256-column buckets."""
    s, _ = _stream(name)
    c0 = int(np.log2(cols))
    base = _matrix(esp, s.m, s.n)
    _append(base, ps.UPDATE, s.I, s.J, s.V, "device")
    base.flush()
    w0 = _what(base)
    assert w0.pairs == 1 and w0.cl_bits == 8, w0
    del base
    cap = ps.plan_cap_for(len(s.J) / s.n, cols)
    for kind in (ps.UPDATE, ps.RAWUPDATE):
        A = _matrix(esp, s.m, s.n, cap=cap)
        ws = _repeat_on_handle(esp, orc, A, s.m, s.n, kind, [(s.I, s.J, s.V)] * 4, "%s cap %.0f" % (name, cap))
        assert ws[0].cl_bits == c0 and ws[0].buckets > w0.buckets and ws[0].predicted == 0, (ws[0], w0)
        for w in ws:
            assert w.pairs == 1 and w.key_bytes == 4 and w.small == 1, w
            assert w.cl_bits in (c0, c0 + 1) and (w.buckets > w0.buckets) == (w.cl_bits < 8), (w, w0)
            # the record and the predicted form: served as soon as a plan repeats
            assert w.predicted == (1 if w.reused else 0), ws
        assert ws[-1].predicted == 1, ws
        if cols < 128:
            assert ws[-1].cl_bits < 8, ws
    # ... and through esp_append_host (the flush's own partition), pinned beside it
    for force in (0, NO_PAIRS):
        A = _matrix(esp, s.m, s.n, force, cap=cap)
        ws = _repeat_on_handle(esp, orc, A, s.m, s.n, ps.UPDATE, [(s.I, s.J, s.V)] * 2, "%s cap %.0f host force %d" % (name, cap, force), how="host")
        for w in ws:
            assert w.pairs == (1 if force == 0 else 0) and w.cl_bits in (c0, c0 + 1), w
        assert ws[0].cl_bits == c0 and ws[0].buckets > w0.buckets, (ws[0], w0)


REFUSED = [("span_refused", "span_served"), ("long_run_first_pair", "ragged_0"), ("long_run_interior_second", "ragged_0"),
           ("long_run_odd_last", "ragged_255")]


@pytest.mark.parametrize("name,after", REFUSED)
def test_refused(esp, orc, name, after):
    """a pair whose rows span exactly 2^19, and a column run of 13 (in the first pair, in the second bucket of an interior pair, in
    the lone bucket of an odd last pair) in a bucket the host's conditions accept: the kernel refuses (its ordinary error-bit
    path), the flush runs again with local_k and equals the oracle; after reset! a stream the pair kernel would serve stays on
    local_k on this handle and equals the oracle."""
    s, _ = _stream(name)
    t, _ = _stream(after)
    assert (s.m, s.n) == (t.m, t.n)
    for kind, how in ((ps.UPDATE, "device"), (ps.RAWUPDATE, "host")):
        want = ps.oracle_csc(orc, s.m, s.n, kind, s.I, s.J, s.V)
        for force in (0, NO_PAIRS):
            A = _matrix(esp, s.m, s.n, force)
            _append(A, kind, s.I, s.J, s.V, how)
            A.flush()
            w = _what(A)
            print(name, "kind", kind, how, "force", force, w)
            assert_csc_equal(A.arrays(), want, "%s kind %d %s force %d:" % (name, kind, how, force))
            assert w.pairs == 0 and w.key_bytes == 4 and w.predicted == 0, w
            if force:
                continue
            A.reset()
            _append(A, kind, t.I, t.J, t.V, how)
            A.flush()
            w = _what(A)
            print(name, "then", after, w)
            assert w.pairs == 0 and w.predicted == 0, w               # (the handle met a pair the kernel refused)
            assert_csc_equal(A.arrays(), ps.oracle_csc(orc, t.m, t.n, kind, t.I, t.J, t.V), "%s after %s:" % (after, name))
        # the same stream on a fresh handle IS served: the refusal above was the stream's, not the shape's
        B = _matrix(esp, t.m, t.n)
        _append(B, kind, t.I, t.J, t.V, how)
        B.flush()
        assert _what(B).pairs == 1


@pytest.mark.parametrize("build,kind", [("repeat_a", ps.UPDATE), ("repeat_a", ps.SET), ("repeat_a", ps.RAWUPDATE), ("repeat_b", ps.UPDATE),
                                        ("repeat_b", ps.COO)])
def test_predicted_same_counts(esp, orc, build, kind):
    """(a) new values, (b) other rows with the same counts: recorded, then served twice ([0, 1, 1]) -- the table is checked by the
    pairs' emitted counts alone, the rows inside are the new batch's"""
    m, n, kind, batches, p = getattr(ps, build)(kind=kind)
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n), m, n, kind, batches, build)
    assert [w.predicted for w in ws] == p["states"] == [0, 1, 1], ws
    assert all(w.pairs == 1 and w.cl_bits == 8 for w in ws) and [w.reused for w in ws] == [0, 1, 1], ws


def test_predicted_same_counts_narrow_buckets(esp, orc):
    """(a) under a cap that cuts buckets of 32 columns: served once the plan has repeated"""
    m, n, kind, batches, p = ps.repeat_a(batches=4)
    cap = ps.plan_cap_for(len(batches[0][1]) / n, 32)
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n, cap=cap), m, n, kind, batches, "repeat_a cap %.0f" % cap)
    assert ws[0].cl_bits == 5 and all(w.pairs == 1 and w.cl_bits < 8 for w in ws), ws
    assert all(w.predicted == (1 if w.reused else 0) for w in ws), ws
    assert ws[0].predicted == 0 and ws[-1].predicted == 1, ws


def test_predicted_counts_cancel_inside_a_pair(esp, orc):
    """(c) kind UPDATE: a position of column a is no longer created, one of column b in the SAME pair is: the pair emits the
    table's count, the flush is served -- and every colptr between a and b has moved by one (checked against the oracle column by
    column, and against the first batch)"""
    m, n, kind, batches, p = ps.repeat_c()
    A = _matrix(esp, m, n)
    cps = []
    states = []
    for i, b in enumerate(batches):
        w = _repeat_on_handle(esp, orc, A, m, n, kind, [b], "repeat_c batch %d" % i)[0]
        states.append(w.predicted)
        assert w.pairs == 1, w
        cps.append(A.arrays()[0].copy())
    assert states == p["states"] == [0, 1, 1], states
    moved = np.zeros(n + 1, np.int64)
    moved[p["a"]:p["b"]] = -1
    assert np.array_equal(cps[1] - cps[0], moved) and np.array_equal(cps[2], cps[1])


def test_predicted_counts_move_between_pairs(esp, orc):
    """(d) the same with a and b in neighbouring pairs: two pairs emit another count -- missed (2: the look-back form's result), then
    served from the table the miss left"""
    m, n, kind, batches, p = ps.repeat_d()
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n), m, n, kind, batches, "repeat_d")
    assert [w.predicted for w in ws] == p["states"] == [0, 2, 1], ws
    assert all(w.pairs == 1 for w in ws), ws


@pytest.mark.parametrize("kind", [ps.UPDATE, ps.RAWUPDATE])
def test_predicted_rows_move_beyond_the_span(esp, orc, kind):
    """(e) a repeat whose rows span 2^19 or more in one pair: pair_pred_k refuses, pair_k refuses, local_k serves (state 2, no pair
    kernel); the next batch of the plan is not predicted and stays on local_k"""
    m, n, kind, batches, p = ps.repeat_e(kind=kind)
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n), m, n, kind, batches, "repeat_e")
    assert [w.predicted for w in ws] == p["states"] == [0, 2, 0], ws
    assert [w.pairs for w in ws] == p["pairs"] == [1, 0, 0], ws


@pytest.mark.parametrize("where", ["first_pair", "odd_last"])
def test_predicted_run_grows_beyond_twelve(esp, orc, where):
    """(g) a repeat in which one column holds 13 entries, bucket by bucket the stream of the batch before: the plan IS reused
    (precondition), pair_pred_k refuses for the run length (pair_count, the phase pair_k shares), pair_k refuses, local_k serves;
    the next batch of the plan is not predicted and stays on local_k"""
    m, n, kind, batches, p = ps.repeat_g(where)
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n), m, n, kind, batches, "repeat_g " + where)
    assert ws[1].reused == 1, ws
    assert [w.predicted for w in ws] == p["states"] == [0, 2, 0], ws
    assert [w.pairs for w in ws] == p["pairs"] == [1, 0, 0], ws


def test_predicted_zeros_move_every_batch(esp, orc):
    """(f) two misses in a row switch the prediction off for the plan: [0, 2, 2, 0]"""
    m, n, kind, batches, p = ps.repeat_f()
    ws = _repeat_on_handle(esp, orc, _matrix(esp, m, n), m, n, kind, batches, "repeat_f")
    assert [w.predicted for w in ws] == p["states"] == [0, 2, 2, 0], ws
    assert all(w.pairs == 1 for w in ws), ws


@pytest.mark.parametrize("rand_mode", [0, 1, 2])
@pytest.mark.parametrize("grid", [(37, 41, 53), (64, 64, 33)])
def test_generator_against_oracle(esp, orc, grid, rand_mode):
    """the device generator on non-cubic grids, UPDATE and RAWUPDATE, seeds A, A, B on one handle: every flush against
    orc.fdrand_stream applied to the oracle; the pair kernel runs, and a flush is served from the table exactly where the
    generator's plan was reused"""
    nx, ny, nz = grid
    N = nx * ny * nz
    for kind in (ps.UPDATE, ps.RAWUPDATE):
        A = _matrix(esp, N, N)
        for i, seed in enumerate((SEED_A, SEED_A, SEED_B)):
            A.reset()
            A.generate_fdrand(nx, ny, nz, seed=seed, rand_mode=rand_mode, kind=kind)
            A.flush()
            w = _what(A)
            print("fdrand", grid, "mode", rand_mode, "kind", kind, "flush", i, w)
            I, J, V = orc.fdrand_stream(nx, ny, nz, rand_mode=rand_mode, seed=seed)
            assert_csc_equal(A.arrays(), ps.oracle_csc(orc, N, N, kind, I, J, V), "fdrand %s mode %d kind %d flush %d:" % (grid, rand_mode, kind, i))
            assert w.pairs == 1 and w.key_bytes == 4 and w.small == 1, (grid, rand_mode, kind, i, w)
            assert w.predicted == (1 if (i and w.reused) else 0), (grid, rand_mode, kind, i, w)
