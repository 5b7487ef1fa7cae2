"""GPU: the boundary to the caller.  Every call that takes a device array is run twice -- once on the host path (NumPy in, NumPy
out) or with freshly allocated tensors, once with every device array replaced by a view at an odd offset between guard bands
(tests/device_views.py) -- and must give the same bits, the same counts and histories, leave every guard element and every input
as it was, and hand back the caller's own view.  The references are the ones the suite already holds the aligned calls to: the
oracle, the C models, the host path.  Nothing rests on a tolerance.

What the views reach that a fresh tensor never does: the scalar side of the three kernels that choose a code path from the
caller's pointer (elem_cells_k<4>, tile_hist_raw_k, the RAW count of run_count_k), bicg_upd_k's plain-double side, and the
elements in front of and behind an array (odd-n tails, chunks padded to 256, outputs written by kernels)."""
import ctypes as C

import numpy as np
import pytest

from bicgstabl_modellib import Model as BicgstablModel
from cg_modellib import Model as CgModel
from device_views import GUARD, bits_of, frozen, guarded
from refmodel import assert_csc_equal, bits

pytestmark = pytest.mark.gpu

SET, UPDATE, RAW, COO = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------------------------- helpers
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def view_of(x, lead):
    """a NumPy array as a guarded device view; .align is its address mod 16"""
    import torch
    g = guarded(dev(x), lead)
    torch.cuda.synchronize()
    return g


def same(got, want, what=""):
    """bit for bit, NumPy arrays or tensors on either side"""
    a, b = bits_of(got), bits_of(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError("%s: element %d of %d differs (%d in all)" % (what, i, len(a), int((a != b).sum())))


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def tridiagonal(esp, n, sym):
    """the matrices of test_small_sizes: (4, -1, -1) for cg, the non-symmetric (4, -1.5 below, -0.5 above) for the others"""
    d = np.arange(1, n + 1)
    lo, up = (-1.0, -1.0) if sym else (-1.5, -0.5)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(UPDATE, np.concatenate([d, d[1:], d[:-1]]), np.concatenate([d, d[:-1], d[1:]]),
             np.concatenate([np.full(n, 4.0), np.full(n - 1, lo), np.full(n - 1, up)]))
    A.flush()
    return A


_CACHE = {}


def matrix(esp, name):
    """built once, never changed: (A, host CSC arrays)"""
    if name not in _CACHE:
        if name == "fd60":
            A = esp.fdrand(5, 4, 3)
        elif name == "fd257":
            A = esp.fdrand(257, 1, 1)
        elif name == "rand257x255":
            rng = np.random.default_rng(11)
            cnt = 3300
            A = esp.ExtendableSparseMatrix(257, 255)
            A.append(UPDATE, rng.integers(1, 258, cnt), rng.integers(1, 256, cnt), rng.standard_normal(cnt))
            A.flush()
        else:
            raise KeyError(name)
        _CACHE[name] = (A, host_arrays(A))
    return _CACHE[name]


@pytest.fixture(scope="module")
def kmodel(tmp_path_factory):
    """(tests/cg_model.c, tests/bicgstabl_model.c)"""
    return CgModel(tmp_path_factory.mktemp("handover_cg")), BicgstablModel(tmp_path_factory.mktemp("handover_bicgstabl"))


@pytest.fixture(scope="module")
def pmodel(tmp_path_factory):
    from precon_modellib import Model
    return Model(tmp_path_factory.mktemp("handover_precon"))


@pytest.fixture(scope="module")
def lmodel(tmp_path_factory):
    from linalg_modellib import Model
    return Model(tmp_path_factory.mktemp("handover_linalg"))


# -------------------------------------------------------------------------------------------------- the proof on the device
def test_a_clobber_on_the_device_is_seen(esp):
    """after a library call that leaves the guards alone, a store from the test itself -- one element behind the view, then one in
    front of it, then into a frozen input -- makes check() raise: what a kernel's stray store would do"""
    A, _ = matrix(esp, "fd60")
    rng = np.random.default_rng(1)
    x = view_of(rng.standard_normal(A.n), 1)
    out = view_of(np.zeros(A.n), 1)
    fx = frozen(x.view)
    assert A.mul(x.view, out.view) is out.view
    A.synchronize()
    x.check(), out.check(), fx.check()
    out.buf[GUARD + 1 + A.n] = 1.0
    with pytest.raises(AssertionError, match=r"offset %d of a view of %d float64" % (A.n, A.n)):
        out.check()
    out.buf[GUARD] = float("nan")            # another NaN than the canary
    with pytest.raises(AssertionError, match=r"offset -1 of"):
        out.check()
    x.view[7] = -x.view[7]
    with pytest.raises(AssertionError, match=r"input element 7 of"):
        fx.check()
    x.check()
    mk = view_of(np.zeros(A.n, np.uint8), 3)
    mk.buf[GUARD + 3 + A.n + 255] = 1
    with pytest.raises(AssertionError, match=r"offset %d of a view of %d uint8" % (A.n + 255, A.n)):
        mk.check()


# ------------------------------------------------------------------------------------------------------------------ vectors
@pytest.mark.parametrize("lo", [0, 1])
@pytest.mark.parametrize("lx", [0, 1])
@pytest.mark.parametrize("name", ["rand257x255", "fd60"])
def test_mul_and_mul_transpose(esp, orc, lmodel, name, lx, lo):
    A, arrays = matrix(esp, name)
    rng = np.random.default_rng(3)
    O = orc.CSC(A.m, A.n, *arrays)
    for fn, nin, nout, ref in ((A.mul, A.n, A.m, O.mul), (A.mul_transpose, A.m, A.n, lambda v: lmodel.mul_transpose(arrays, v))):
        v = rng.standard_normal(nin)
        want = fn(v)                                             # the host path
        same(want, ref(v), fn.__name__ + " host path against its model")
        x, out = view_of(v, lx), view_of(np.full(nout, 7.0), lo)
        assert (x.align, out.align) == (8 * lx, 8 * lo)
        fx = frozen(x.view)
        got = fn(x.view, out.view)
        A.synchronize()
        assert got is out.view
        same(got, want, fn.__name__)
        x.check("x"), out.check("out"), fx.check("x")


def interleaved(n):
    return [range(1, n + 1, 2), range(2, n + 1, 2)]


PRECONS = {
    "jacobi": lambda esp, A: esp.JacobiPreconditioner(A),
    "ilu0": lambda esp, A: esp.ILU0Preconditioner(A),
    "parallel_ilu0": lambda esp, A: esp.ParallelILU0Preconditioner(A),
    "iluam": lambda esp, A: esp.ILUAMPreconditioner(A),
    "iluk2": lambda esp, A: esp.ILUKPreconditioner(A, 2),
    "ilut": lambda esp, A: esp.ILUTPreconditioner(A),
    "colored": lambda esp, A: esp.ColoredPreconditioner(A),
    "block_ilu0_permuted": lambda esp, A: esp.BlockPreconditioner(A, interleaved(A.n), esp.ILU0Preconditioner),
    "block_jacobi_identity": lambda esp, A: esp.BlockPreconditioner(A, [range(1, 31), range(31, A.n + 1)], esp.JacobiPreconditioner),
    "spai0": lambda esp, A: esp.SPAIPreconditioner(A, order=0),
    "spai1": lambda esp, A: esp.SPAIPreconditioner(A, order=1),
    "amg": lambda esp, A: esp.AMGPreconditioner(A, max_coarse=16),
    "rsamg": lambda esp, A: esp.RS_AMGPreconditioner(A, max_coarse=16),
    "lu_columns": lambda esp, A: esp.LUFactorization(A, leaf_size=8),
    "lu_panels": lambda esp, A: esp.LUFactorization(A, leaf_size=8, form="panels"),
    "cholesky": lambda esp, A: esp.CholeskyFactorization(A, leaf_size=8),
}


@pytest.mark.parametrize("name", ["fd60", "fd257"])
@pytest.mark.parametrize("kind", sorted(PRECONS))
def test_ldiv(esp, pmodel, kind, name):
    """P.ldiv(v, out) of every preconditioner class: v and out at leads (0, 1), (1, 0), (1, 1), and out is v as one view"""
    A, arrays = matrix(esp, name)
    P = PRECONS[kind](esp, A)
    try:
        v = np.random.default_rng(5).standard_normal(A.n)
        want = P.ldiv(v)                                         # the host path
        if kind == "jacobi":
            same(want, pmodel.jacobi_ldiv(A.jacobi(), v), "host path against precon_model.c")
        if kind == "ilu0":
            same(want, pmodel.ilu0_ldiv(arrays, *A.ilu0(), v), "host path against precon_model.c")
        for lv, lu in ((0, 1), (1, 0), (1, 1)):
            x, out = view_of(v, lv), view_of(np.full(A.n, 7.0), lu)
            assert (x.align, out.align) == (8 * lv, 8 * lu)
            fx = frozen(x.view)
            got = P.ldiv(x.view, out.view)
            A.synchronize()
            assert got is out.view
            same(got, want, "%s leads (%d, %d)" % (kind, lv, lu))
            x.check("v"), out.check("out"), fx.check("v")
        x = view_of(v, 1)
        got = P.ldiv(x.view, x.view)                             # in place
        A.synchronize()
        assert got is x.view and x.align == 8
        same(got, want, kind + " in place")
        x.check("v = out")
    finally:
        P.close()


SOLVERS = ["cg", "bicgstabl1", "bicgstabl2", "bicgstabl4", "gmres_mgs", "gmres_cgs", "gmres_dgks", "simple"]
LEADS3 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]   # b, x, r_shadow -- each on its own and all together


def solve(esp, solver, A, P, b, x, r_shadow):
    """one truncated run (the limits of the existing truncation tests) -> (x, what the call reports besides x)"""
    if solver == "cg":
        x, log = esp.cg(A, b, Pl=P, x=x, maxiter=7, log=True)
    elif solver.startswith("bicgstabl"):
        l = int(solver[-1])
        x, log = esp.bicgstabl(A, b, l=l, Pl=P, x=x, r_shadow=r_shadow, max_mv_products=6 * l, reltol=0.0, log=True)
    elif solver.startswith("gmres"):
        x, log = esp.gmres(A, b, Pl=P, x=x, restart=5, maxiter=7, reltol=0.0, orth_meth=solver[6:], log=True)
    else:
        x, log = esp.simple(A, b, u=x, Pl=P, maxiter=5, reltol=0.0, log=True)
    return x, log


def same_log(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            same(got[k], want[k], "%s: %s" % (what, k))
        elif isinstance(want[k], float):
            assert bits(np.array([got[k]]))[0] == bits(np.array([want[k]]))[0], (what, k, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


SOLVER_LEADS = [(s, l) for s in SOLVERS for l in LEADS3 if s.startswith("bicgstabl") or not l[2] or l == (1, 1, 1)]


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 513])
@pytest.mark.parametrize("solver,leads", SOLVER_LEADS, ids=["%s-b%dx%ds%d" % ((s,) + l) for s, l in SOLVER_LEADS])
def test_solvers(esp, orc, kmodel, solver, leads, n):
    """cg!, bicgstabl!, gmres! and simple! from a random start: b (unchanged), x (updated in place, the returned object) and
    r_shadow as views at `leads` (only bicgstabl takes an r_shadow: the others run its lead with all three); both parities of n on
    each side of a 256 chunk, n >> 1 == 0, the scalar tails"""
    lb, lx, ls = leads
    A = tridiagonal(esp, n, sym=solver == "cg")
    arrays = host_arrays(A)
    rng = np.random.default_rng(100 + n)
    b, x0, rsh = rng.standard_normal(n), rng.standard_normal(n), rng.random(n)
    shadow = solver.startswith("bicgstabl")
    for kind in (["jacobi", "ilu0"] if solver == "simple" else ["identity", "jacobi", "ilu0"]):
        P = {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner}[kind](A)
        try:
            hx = x0.copy()
            wx, wlog = solve(esp, solver, A, P, b, hx, rsh if shadow else None)          # the host path
            assert wx is hx
            if n == 257 and solver == "cg":
                mx, mh, mit, mconv = kmodel[0].cg(kmodel[0].precon(kind, arrays, orc), arrays, b, x=x0, maxiter=7)
                same(wx, mx, "host path against cg_model.c")
                same(np.concatenate([[wlog["r0"]], wlog["resnorm"]]), mh, "history against cg_model.c")
                assert (wlog["iters"], wlog["isconverged"]) == (mit, mconv)
            if n == 257 and shadow:
                l = int(solver[-1])
                mx, mh, mit, mmv, mconv = kmodel[1].bicgstabl(kmodel[1].precon(kind, arrays, orc), arrays, b, l=l, x=x0,
                                                              max_mv_products=6 * l, reltol=0.0, r_shadow=rsh)
                same(wx, mx, "host path against bicgstabl_model.c")
                same(np.concatenate([[wlog["r0"]], wlog["resnorm"]]), mh, "history against bicgstabl_model.c")
                assert (wlog["iters"], wlog["mvps"], wlog["isconverged"]) == (mit, mmv, mconv)
            vb, vx = view_of(b, lb), view_of(x0, lx)
            vs = view_of(rsh, ls) if shadow else None
            assert (vb.align, vx.align) == (8 * lb, 8 * lx) and (vs is None or vs.align == 8 * ls)
            fb, fs = frozen(vb.view), frozen(vs.view) if shadow else None
            gx, glog = solve(esp, solver, A, P, vb.view, vx.view, vs.view if shadow else None)
            A.synchronize()
            what = "%s %s n=%d leads (%d, %d, %d)" % (solver, kind, n, lb, lx, ls)
            assert gx is vx.view, what
            same(gx, wx, what)
            same_log(glog, wlog, what)
            vb.check(what + " b"), vx.check(what + " x"), fb.check(what + " b")
            if shadow:
                vs.check(what + " r_shadow"), fs.check(what + " r_shadow")
        finally:
            if P is not None:
                P.close()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", ["rand257x255", "fd60"])
def test_diag_scale(esp, name, side):
    A, _ = matrix(esp, name)
    d = np.random.default_rng(9).standard_normal(A.m if side == "left" else A.n)
    want = A.diag_scale(d, side=side).sparse().arrays()
    v = view_of(d, 1)
    fd = frozen(v.view)
    assert v.align == 8
    got = A.diag_scale(v.view, side=side)
    assert_csc_equal(got.sparse().arrays(), want, "diag_scale " + side)
    v.check("d"), fd.check("d")


# --------------------------------------------------------------------------------------------------------- assembly input
def oracle_csc(orc, m, n, kinds, I, J, V, sub=False):
    kinds = np.asarray(kinds, np.uint8)
    if sub:
        V = np.where(kinds == SET, V, -V)
    if (kinds == COO).all():
        return orc.sparse_coo(I, J, V, m, n).arrays()
    O = orc.ExtendableSparseMatrix(m, n)
    O.apply(kinds, I, J, V)
    O.flush()
    return O.arrays()


def appended(esp, m, n, kind, I, J, V, kinds, op, leads, hook=None):
    """one append_device + flush with the arrays at `leads` (I, J, V, kinds; None: fresh tensors) -> (A, what the flush and the
    append report); inputs and guards checked"""
    import torch
    A = esp.ExtendableSparseMatrix(m, n)
    if hook:
        hook(A)
    if leads is None:
        args = [dev(I), dev(J), dev(V)] + ([dev(kinds)] if kinds is not None else [])
        torch.cuda.synchronize()
        gs = []
    else:
        gs = [view_of(a, l) for a, l in zip((I, J, V) + ((kinds,) if kinds is not None else ()), leads)]
        args = [g.view for g in gs]
        for g, l, a in zip(gs, leads, args):
            assert g.align == (l * a.element_size()) % 16
    fz = [frozen(a) for a in args]
    A.append_device(kind, args[0], args[1], args[2], op=op, kinds=args[3] if kinds is not None else None)
    route = (A.debug_last_append_route(), A.debug_last_plan_reused())
    A.flush()
    A.synchronize()
    for f in fz:
        f.check("append_device input")
    for g in gs:
        g.check("append_device input")
    return A, route + (A.debug_last_partition(), A.debug_last_path())


@pytest.mark.parametrize("count", [1, 2, 255, 257])
def test_append_device_in_stream_order(esp, orc, count):
    """esp_append_device below the partitioning routes (pack_k reads the four arrays entry by entry): every kind, a kinds array,
    op "-"; each array misaligned on its own and all together"""
    rng = np.random.default_rng(count)
    m, n = 300, 200
    I, J, V = rng.integers(1, m + 1, count), rng.integers(1, n + 1, count), rng.standard_normal(count)
    mixed = rng.integers(0, 3, count).astype(np.uint8)
    for kind, kinds, op in ((SET, None, "+"), (UPDATE, None, "+"), (RAW, None, "+"), (COO, None, "+"), (0, mixed, "+"), (UPDATE, None, "-"),
                            (0, mixed, "-")):
        kk = np.full(count, kind, np.uint8) if kinds is None else kinds
        want = oracle_csc(orc, m, n, kk, I, J, V, sub=op == "-")
        nargs = 3 if kinds is None else 4
        alone = [tuple(int(q == p) for q in range(nargs)) for p in range(nargs)]
        every = [None, (0,) * nargs] + alone + [(1, 1, 1, 3)[:nargs], (1, 1, 1, 7)[:nargs]]
        for leads in dict.fromkeys(every):
            A, what = appended(esp, m, n, kind, I, J, V, kinds, op, leads)
            assert what[0] == 1, what                          # packed in stream order
            assert_csc_equal(A.sparse().arrays(), want, "count %d kind %d op %s leads %s" % (count, kind, op, leads))


def presorted_stream(count, n, seed):
    rng = np.random.default_rng(seed)
    J = np.sort(rng.integers(1, n + 1, count))
    I = np.clip(J + rng.integers(-40, 41, count), 1, n)
    return I, J, rng.standard_normal(count)


PART_N, PART_COUNT = 1 << 17, 1_100_001


@pytest.fixture(scope="module")
def presorted(orc):
    """a pre-sorted stream of 1 100 001 entries over 2^17 columns with its oracle result (computed once)"""
    I, J, V = presorted_stream(PART_COUNT, PART_N, 17)
    return I, J, V, oracle_csc(orc, PART_N, PART_N, np.full(PART_COUNT, UPDATE, np.uint8), I, J, V)


@pytest.mark.parametrize("leads", [None, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_append_partitioned(esp, presorted, leads):
    """the append that is the partition (partition.hip, append_partitioned) on a pre-sorted stream of an odd count with 9 planned
    prefix bits -- the plan of the existing test of this route (test_append_device_reuses_the_previous_run_lists), whose second
    assembly repeats it: 2^9 buckets of 0.9 * 4096 entries hold 1.9 million, and from its second flush on a handle takes a bit off
    the plan where 2^8 buckets would do within 2 %, so the count stays above 1.08 * 2^8 * 4096 for the repetition to find its plan.
    run_count_k<RAW> reads the caller's columns in pairs or singly by J's address, and `vec` also changes which entry a lane's
    item k is; the scatter reads I, J and V.  The same stream again takes the plan-reuse branch over misaligned arrays too.
    Read-outs: esp_debug_last_append_route 2, then 3 (= esp_debug_last_plan_reused 1); esp_debug_last_partition 4."""
    I, J, V, want = presorted
    assert PART_COUNT % 2 == 1 and PART_COUNT > 4096
    A, what = appended(esp, PART_N, PART_N, UPDATE, I, J, V, None, "+", leads)
    assert what[:3] == (2, 0, 4), (leads, what)
    assert_csc_equal(A.sparse().arrays(), want, "partitioned, leads %s" % (leads,))
    # the same stream again on the same handle: over the kept run lists
    gs = [view_of(a, l) for a, l in zip((I, J, V), leads or (0, 0, 0))]
    fz = [frozen(g.view) for g in gs]
    A.reset()
    A.append_device(UPDATE, *[g.view for g in gs])
    again = (A.debug_last_append_route(), A.debug_last_plan_reused())
    A.flush()
    A.synchronize()
    assert again == (3, 1) and A.debug_last_partition() == 4, (leads, again)
    assert_csc_equal(A.sparse().arrays(), want, "partitioned over kept run lists, leads %s" % (leads,))
    for g, f in zip(gs, fz):
        g.check("repeated append"), f.check("repeated append")


FIRST_COUNT = (1 << 18) + 1


@pytest.fixture(scope="module")
def shuffled(orc):
    """2^18 + 1 shuffled entries over 3000 x 70001 with their oracle result (computed once)"""
    rng = np.random.default_rng(29)
    m, n = 3000, 70001
    I, J, V = rng.integers(1, m + 1, FIRST_COUNT), rng.integers(1, n + 1, FIRST_COUNT), rng.standard_normal(FIRST_COUNT)
    return m, n, I, J, V, oracle_csc(orc, m, n, np.full(FIRST_COUNT, RAW, np.uint8), I, J, V)


@pytest.mark.parametrize("leads", [None, (0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)])
def test_append_first_pass(esp, shuffled, leads):
    """a shuffled stream of 2^18 + 1 entries: the first radix pass of the flush runs from the caller's arrays (partition.hip,
    append_first_pass; esp_debug_last_append_route 5).  tile_hist_raw_k reads the columns in pairs (J aligned: the odd tail of
    its pair branch is the last entry) or singly (J misaligned); the scatter reads I, J and V.  J aligned with I and V misaligned,
    and J misaligned."""
    m, n, I, J, V, want = shuffled
    A, what = appended(esp, m, n, RAW, I, J, V, None, "+", leads, lambda A: A.debug_plan_cap(300.0))
    print("leads", leads, "route, plan reused, partition, path:", what)
    assert what[0] == 5, what
    assert_csc_equal(A.sparse().arrays(), want, "first pass, leads %s" % (leads,))


def random_cells(nloc, nc, n, seed):
    """cells of distinct nodes, random element matrices and diagonal terms, in append_elements' host layouts (Fortran order)"""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, n - 64, nc)
    cn = np.empty((nloc, nc), np.int64, order="F")
    for c in range(nc):
        cn[:, c] = 1 + start[c] + rng.choice(64, nloc, replace=False)
    return cn, np.asfortranarray(rng.standard_normal((nloc, nloc, nc))), np.asfortranarray(rng.standard_normal((nloc, nc)))


def shaped(g, *shape):
    """the guarded flat view in the device layout of append_elements: a tensor of shape (ncells, nloc[, nloc]) whose C order is
    Julia's column-major (nloc[, nloc], ncells)"""
    t = g.view.reshape(*shape)
    assert t.data_ptr() == g.view.data_ptr() and t.is_contiguous()
    return t


ELEMENT_LEADS = [(True, l) for l in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]] + \
                [(False, l) for l in [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)]]


@pytest.mark.parametrize("nc", [1, 257, 1000])
@pytest.mark.parametrize("diag,leads", ELEMENT_LEADS, ids=["%s-c%dd%de%d" % (("diag" if d else "nodiag",) + l) for d, l in ELEMENT_LEADS])
@pytest.mark.parametrize("nloc", [3, 4])
def test_append_elements(esp, orc, nloc, diag, leads, nc):
    """esp_append_elements with cellnodes, elmat and diag as views at `leads` (read at FLUSH time: kept until then): the four alignment
    combinations of cellnodes x diag -- elem_cells_k<4> takes 16-byte loads only when both are aligned --, elmat misaligned, against
    the host entry point and the oracle; then the kept plan with elmat and diag of esp_append_elements_again as views.
    esp_debug_last_append_route names the kernel that read the arrays: 7 elem_cells_k (more than 4096 updates), 8 elem_stream_k."""
    n = 5000
    cn, em, dg = random_cells(nloc, nc, n, 7 * nloc + nc)
    dgu = dg if diag else None
    Is, Js, Vs = orc.elements_stream(cn, em, dgu)
    want = oracle_csc(orc, n, n, np.full(len(Is), RAW, np.uint8), Is, Js, Vs)
    H = esp.ExtendableSparseMatrix(n, n)
    H.append_elements(cn, em, dgu)                                # the host entry point
    H.flush()
    assert_csc_equal(H.sparse().arrays(), want, "host entry point")
    route = 7 if len(Is) > 4096 else 8
    em2, dg2 = np.asfortranarray(em * 1.7), np.asfortranarray(dg * 0.3)
    I2, J2, V2 = orc.elements_stream(cn, em2, dg2 if diag else None)
    O2 = orc.ExtendableSparseMatrix(n, n)
    O2.apply(np.full(len(Is), RAW, np.uint8), Is, Js, Vs)
    O2.flush()
    O2.apply(np.full(len(I2), RAW, np.uint8), I2, J2, V2)
    O2.flush()
    want2 = O2.arrays()
    lc, ld, le = leads
    gc, ge = view_of(cn.ravel(order="F"), lc), view_of(em.ravel(order="F"), le)
    gd = view_of(dg.ravel(order="F"), ld) if diag else None
    assert (gc.align, ge.align) == (8 * lc, 8 * le) and (gd is None or gd.align == 8 * ld)
    held = [g for g in (gc, ge, gd) if g is not None]
    fz = [frozen(g.view) for g in held]
    A = esp.ExtendableSparseMatrix(n, n)
    A.elements_keep_plan(1)
    A.append_elements(shaped(gc, nc, nloc), shaped(ge, nc, nloc, nloc), shaped(gd, nc, nloc) if diag else None)
    assert A.debug_last_append_route() == route, (A.debug_last_append_route(), route)
    A.flush()
    A.synchronize()
    what = "nloc %d diag %s ncells %d leads (%d, %d, %d)" % (nloc, diag, nc, lc, ld, le)
    assert_csc_equal(A.sparse().arrays(), want, what)
    for g, f in zip(held, fz):
        g.check(what), f.check(what)
    if route == 7:                                            # (only the item partition leaves a plan)
        ge2 = view_of(em2.ravel(order="F"), 1 - le)
        gd2 = view_of(dg2.ravel(order="F"), 1 - ld) if diag else None
        held = [g for g in (ge2, gd2) if g is not None]
        fz = [frozen(g.view) for g in held]
        A.append_elements_again(shaped(ge2, nc, nloc, nloc), shaped(gd2, nc, nloc) if diag else None)
        A.flush()
        A.synchronize()
        assert_csc_equal(A.sparse().arrays(), want2, what + " again")
        for g, f in zip(held, fz):
            g.check(what + " again"), f.check(what + " again")
    else:
        with pytest.raises(esp.EspError):
            A.append_elements_again(shaped(ge, nc, nloc, nloc), shaped(gd, nc, nloc) if diag else None)


@pytest.mark.parametrize("dim,npd", [(2, 7), (3, 4), (2, 18)])
def test_generate_fem_mesh(esp, orc, dim, npd):
    """esp_generate_fem_mesh fills caller-owned arrays: cellnodes, elmat and diag as views must hold the aligned run's bits -- the
    oracle's mesh -- and nothing beside them may change"""
    import torch
    nloc = dim + 1
    DT = (np.int64, np.float64, np.float64)
    cn, em, dg = orc.fem_mesh(dim, npd, seed=0x5EED0004, order_mode=1, node_mode=1)
    nc = cn.shape[1]
    A = esp.ExtendableSparseMatrix(npd ** dim, npd ** dim)
    fresh = [torch.full((nc * nloc,), -7, dtype=torch.int64, device="cuda"),
             torch.full((nc * nloc * nloc,), -7.0, dtype=torch.float64, device="cuda"),
             torch.full((nc * nloc,), -7.0, dtype=torch.float64, device="cuda")]
    torch.cuda.synchronize()
    A.generate_fem_mesh(dim, npd, *fresh, seed=0x5EED0004, order_mode=1, node_mode=1)
    A.synchronize()
    for got, want in zip(fresh, (cn, em, dg)):
        same(got, want.ravel(order="F"), "aligned run against the oracle's mesh")
    for leads in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        gs = [view_of(np.full(t.numel(), -7, dt), l) for t, dt, l in zip(fresh, DT, leads)]
        A.generate_fem_mesh(dim, npd, gs[0].view, gs[1].view, gs[2].view, seed=0x5EED0004, order_mode=1, node_mode=1)
        A.synchronize()
        for g, t, l in zip(gs, fresh, leads):
            assert g.align == 8 * l
            same(g.view, t, "leads %s" % (leads,))
            g.check("leads %s" % (leads,))
    # without the diagonal term
    gs = [view_of(np.full(t.numel(), -7, dt), 1) for t, dt in zip(fresh[:2], DT)]
    A.generate_fem_mesh(dim, npd, gs[0].view, gs[1].view, None, seed=0x5EED0004, order_mode=1, node_mode=1)
    A.synchronize()
    for g, t in zip(gs, fresh):
        same(g.view, t, "no diag")
        g.check("no diag")


# ------------------------------------------------------------------------------------------ device outputs through the C ABI
def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def dp(t):
    return C.c_void_p(t.data_ptr())


class Out:
    """one output array of a call: dtype, count and the lead of its device view"""

    def __init__(self, dtype, count, lead):
        self.dtype, self.count, self.lead = np.dtype(dtype), int(count), lead


def both(call, outs, what):
    """call(pointers, on_device) once into NumPy arrays and once into guarded device views at the given leads: the same bits, the
    guards intact -> the host arrays"""
    host = [np.full(o.count, 9, o.dtype) for o in outs]
    assert call([vp(h) for h in host], 0) == 0, what
    gs = [view_of(np.full(o.count, 5, o.dtype), o.lead) for o in outs]
    for g, o in zip(gs, outs):
        assert g.align == (o.lead * o.dtype.itemsize) % 16
    assert call([dp(g.view) for g in gs], 1) == 0, what
    import torch
    torch.cuda.synchronize()
    for k, (g, h) in enumerate(zip(gs, host)):
        same(g.view, h, "%s output %d" % (what, k))
        g.check("%s output %d" % (what, k))
    return host


def with_dirichlet(esp, name):
    """a copy of the matrix with every seventh diagonal entry at the penalty"""
    A, _ = matrix(esp, name)
    B = A.copy()
    idx = np.arange(1, B.n + 1, 7)
    B.append(SET, idx, idx, np.full(len(idx), 1.0e30))
    B.flush()
    return B


def readouts(esp, A):
    """(name, set-up -> (object to close or None, call, outs)) for every call that writes a device array a caller owns"""
    lib, h, n = A._d.lib, A._d.h, A.n
    nnz = A.nnz()
    i8, i4, f8, u1 = np.int64, np.int32, np.float64, np.uint8

    def precon(make, then):
        def setup():
            P = make()
            name_call_outs = then(P)
            return P, name_call_outs[0], name_call_outs[1]
        return setup

    def nnz_of(handle):
        z = C.c_int64()
        assert lib.esp_nnz(handle, C.byref(z)) == 0
        return z.value

    def amg_n(P, level):
        a, nl = C.c_void_p(), C.c_int64()
        assert lib.esp_precon_amg_level(P._p, level, C.byref(a), None, C.byref(nl), None, None) == 0
        return nl.value

    nc = C.c_int64()
    table = [
        ("esp_mark_dirichlet", lambda: (None, lambda p, d: lib.esp_mark_dirichlet(h, 1.0e20, p[0], d), [Out(u1, n, 3)])),
        ("esp_mark_dirichlet lead 7", lambda: (None, lambda p, d: lib.esp_mark_dirichlet(h, 1.0e20, p[0], d), [Out(u1, n, 7)])),
        ("esp_jacobi_setup", lambda: (None, lambda p, d: lib.esp_jacobi_setup(h, p[0], d), [Out(f8, n, 1)])),
        ("esp_ilu0_setup", lambda: (None, lambda p, d: lib.esp_ilu0_setup(h, p[0], p[1], d), [Out(f8, n, 1), Out(i8, n, 1)])),
        ("esp_ilu0_setup idiag alone", lambda: (None, lambda p, d: lib.esp_ilu0_setup(h, p[0], p[1], d), [Out(f8, n, 0), Out(i8, n, 1)])),
        ("esp_graph_coloring", lambda: (None, lambda p, d: lib.esp_graph_coloring(h, C.byref(nc), p[0], d), [Out(i8, n, 1)])),
        ("esp_nested_dissection", lambda: (None, lambda p, d: lib.esp_nested_dissection(h, 8, 48, p[0], p[1], d),
                                           [Out(i8, n, 1), Out(i4, n, 1)])),
        ("esp_nested_dissection level lead 3", lambda: (None, lambda p, d: lib.esp_nested_dissection(h, 8, 48, p[0], p[1], d),
                                                        [Out(i8, n, 0), Out(i4, n, 3)])),
        ("esp_precon_get_factor iluam", precon(lambda: esp.ILUAMPreconditioner(A), lambda P: (
            lambda p, d: lib.esp_precon_get_factor(P._p, p[0], d), [Out(f8, nnz, 1)]))),
        ("esp_precon_get_factor spai1", precon(lambda: esp.SPAIPreconditioner(A, order=1), lambda P: (
            lambda p, d: lib.esp_precon_get_factor(P._p, p[0], d), [Out(f8, len(P.factor()), 1)]))),
        ("esp_precon_colored_colors", precon(lambda: esp.ColoredPreconditioner(A), lambda P: (
            lambda p, d: lib.esp_precon_colored_colors(P._p, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_colored_perm", precon(lambda: esp.ColoredPreconditioner(A), lambda P: (
            lambda p, d: lib.esp_precon_colored_perm(P._p, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_iluk_levels", precon(lambda: esp.ILUKPreconditioner(A, 2), lambda P: (
            lambda p, d: lib.esp_precon_iluk_levels(P._p, p[0], d), [Out(i4, P.stats()["nnz"], 1)]))),
        ("esp_precon_iluk_levels lead 3", precon(lambda: esp.ILUKPreconditioner(A, 2), lambda P: (
            lambda p, d: lib.esp_precon_iluk_levels(P._p, p[0], d), [Out(i4, P.stats()["nnz"], 3)]))),
        ("esp_precon_amg_aggregates", precon(lambda: esp.AMGPreconditioner(A, max_coarse=16), lambda P: (
            lambda p, d: lib.esp_precon_amg_aggregates(P._p, 0, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_amg_splitting", precon(lambda: esp.RS_AMGPreconditioner(A, max_coarse=16), lambda P: (
            lambda p, d: lib.esp_precon_amg_splitting(P._p, 0, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_amg_coarse_inverse", precon(lambda: esp.AMGPreconditioner(A, max_coarse=16), lambda P: (
            lambda p, d: lib.esp_precon_amg_coarse_inverse(P._p, p[0], d), [Out(f8, amg_n(P, P.levels - 1) ** 2, 1)]))),
        ("esp_precon_lu_perm", precon(lambda: esp.LUFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_lu_perm(P._p, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_lu_tree", precon(lambda: esp.LUFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_lu_tree(P._p, p[0], p[1], d), [Out(i4, n, 1), Out(i8, n, 1)]))),
        ("esp_precon_lu_tree level lead 3", precon(lambda: esp.LUFactorization(A, leaf_size=8, form="panels"), lambda P: (
            lambda p, d: lib.esp_precon_lu_tree(P._p, p[0], p[1], d), [Out(i4, n, 3), Out(i8, n, 0)]))),
        ("esp_precon_get_factor lu panels", precon(lambda: esp.LUFactorization(A, leaf_size=8, form="panels"), lambda P: (
            lambda p, d: lib.esp_precon_get_factor(P._p, p[0], d), [Out(f8, len(P.factor()), 1)]))),
        ("esp_precon_cholesky_perm", precon(lambda: esp.CholeskyFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_cholesky_perm(P._p, p[0], d), [Out(i8, n, 1)]))),
        ("esp_precon_cholesky_tree", precon(lambda: esp.CholeskyFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_cholesky_tree(P._p, p[0], p[1], d), [Out(i4, n, 3), Out(i8, n, 1)]))),
        ("esp_precon_cholesky_factor colptr", precon(lambda: esp.CholeskyFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_cholesky_factor(P._p, p[0], None, None, d), [Out(i8, n + 1, 1)]))),
        ("esp_precon_cholesky_factor rows and values", precon(lambda: esp.CholeskyFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_cholesky_factor(P._p, None, p[0], p[1], d),
            [Out(i8, len(P.factor()[1]), 1), Out(f8, len(P.factor()[1]), 1)]))),
        ("esp_precon_cholesky_factor all three", precon(lambda: esp.CholeskyFactorization(A, leaf_size=8), lambda P: (
            lambda p, d: lib.esp_precon_cholesky_factor(P._p, p[0], p[1], p[2], d),
            [Out(i8, n + 1, 1), Out(i8, len(P.factor()[1]), 0), Out(f8, len(P.factor()[1]), 1)]))),
    ]
    return table


READOUT_COUNT = 26


@pytest.mark.parametrize("k", range(READOUT_COUNT))
@pytest.mark.parametrize("name", ["fd60", "fd257"])
def test_device_outputs(esp, name, k):
    """every call that writes a device array a caller owns: into a guarded view at a non-zero lead it gives the bits of its
    host-output twin and touches nothing beside the view (int32 outputs at leads 1 and 3, uint8 at 3 and 7)"""
    A = with_dirichlet(esp, name) if k < 2 else matrix(esp, name)[0]
    table = readouts(esp, A)
    assert len(table) == READOUT_COUNT
    what, setup = table[k]
    P, call, outs = setup()
    try:
        host = both(call, outs, what + " " + name)
        if k < 2:
            assert host[0].sum() == len(range(0, A.n, 7))         # (the marker is not trivially empty)
    finally:
        if P is not None:
            P.close()


@pytest.mark.parametrize("lead", [1, 3, 7])
@pytest.mark.parametrize("name", ["fd60", "fd257"])
def test_eliminate_dirichlet_reads_a_misaligned_marker(esp, orc, name, lead):
    B = with_dirichlet(esp, name)
    marker = B.mark_dirichlet()
    assert marker.sum() == len(range(0, B.n, 7))
    want = orc.CSC(B.m, B.n, *host_arrays(B)).eliminate_dirichlet(marker).arrays()
    H = B.copy().eliminate_dirichlet(marker)                      # the host path
    assert_csc_equal(H.sparse().arrays(), want, "host path against the oracle")
    g = view_of(marker.astype(np.uint8), lead)
    f = frozen(g.view)
    assert g.align == lead
    D = B.copy()
    D.flush()
    D._d.ck(D._d.lib.esp_eliminate_dirichlet(D._d.h, dp(g.view), 1))
    D._touch()
    assert_csc_equal(D.sparse().arrays(), want, "marker at lead %d" % lead)
    g.check("marker"), f.check("marker")


@pytest.mark.parametrize("leads", [(1, 0), (0, 1), (1, 1)])
def test_shard_export(esp, leads):
    """esp_shard_export with P = 3 writes the pending entries, packed, into the caller's keys and vals: as views they hold the
    aligned export's bits, the offsets agree, the guards are intact"""
    import torch
    rng = np.random.default_rng(13)
    N, cnt = 4000, 9001
    A = esp.ExtendableSparseMatrix(N, N)
    A.append(UPDATE, rng.integers(1, N + 1, cnt), rng.integers(1, N + 1, cnt), rng.standard_normal(cnt))
    d = A._d
    d.commit()
    assert d.pending() == cnt
    keys, vals = torch.full((cnt,), -7, dtype=torch.int64, device="cuda"), torch.full((cnt,), -7.0, dtype=torch.float64, device="cuda")
    offs = np.zeros(4, np.int64)
    torch.cuda.synchronize()
    d.ck(d.lib.esp_shard_export(d.h, 3, dp(keys), dp(vals), vp(offs)))
    A.synchronize()
    assert offs[0] == 0 and offs[3] == cnt and (np.diff(offs) > 0).all()
    gk, gv = view_of(np.full(cnt, -7, np.int64), leads[0]), view_of(np.full(cnt, -7.0), leads[1])
    offs2 = np.zeros(4, np.int64)
    d.ck(d.lib.esp_shard_export(d.h, 3, dp(gk.view), dp(gv.view), vp(offs2)))
    A.synchronize()
    assert (gk.align, gv.align) == (8 * leads[0], 8 * leads[1]) and np.array_equal(offs, offs2)
    same(gk.view, keys, "keys"), same(gv.view, vals, "vals")
    gk.check("keys"), gv.check("vals")
