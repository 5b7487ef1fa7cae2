"""GPU: restarted GMRES for several right-hand sides -- gmres(A, B) with an (n, k) B (include/esparse_hip.h, esp_gmres_many;
DESIGN.md 5v).  The contract is one sentence: for every column r, x[:, r], the whole residual history of r, its iteration,
product and correction-pass counts and its converged flag are bit for bit what the single call gives for column r alone -- whatever
the other columns of the chunk hold and whenever they stop.  Where tests/gmres_model.c has the kind (Identity, Jacobi, ILU0, ILUAM)
the columns are held to the model as well.

The constants and the sizes that straddle them:
  MC = 8        columns of a chunk (ESP_MANY_CHUNK).  Column counts k: 2, 7, 8, 9, 17.
  KT = 256      elements of a chunk of the summation shape; the MGS step takes two chunks a round: n in 1, 2, 3, 255, 256, 257, 513,
                and 65537, where the second level has two groups.
  GM_GROUP = 8  trees of a group of the batched dot products: restart 1, 2, 5 (one group), 9 (two), 17 (three), 64 (eight, the cap).
  KCAP = 2048   entries of a row slice a workgroup stages in LDS: test_cg_many_gpu's band matrices, made non-symmetric."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from bicgstabl_modellib import convdiff_triplets
from device_views import frozen
from edge_patterns import from_triplets, tridiagonal
from gmres_modellib import RELTOL, Model
from refmodel import bits
from test_cg_many_gpu import (MC, KS, KMAX, ORDERS, PRECONS, band_matrix, close, dev_ptr, from_scipy, history_of, host_arrays, pads_intact,
                              same_bits, staggered_columns, strided, to_device, to_host)

pytestmark = pytest.mark.gpu

ESP_OK, ESP_ERR_INVALID, ESP_ERR_STATE = 0, -1, -6
ORTHS = ["mgs", "cgs", "dgks"]
ORTH_CODE = {"mgs": 0, "cgs": 1, "dgks": 2}
FUSED = ["identity", "jacobi", "ilu0"]
KEYS = ["isconverged", "iters", "mvps", "r0", "reorth", "resnorm"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("gmres_many_model"))


def convdiff(esp, pe, dims=(10, 10, 10)):
    return from_triplets(esp, dims[0] * dims[1] * dims[2], *convdiff_triplets(*dims, pe))


def single_calls(esp, A, P, B, X0=None, **kw):
    """the single call on every column: [(x, history, iters, mvps, reorth, isconverged)]"""
    out = []
    for r in range(B.shape[1]):
        x0 = None if X0 is None else np.ascontiguousarray(X0[:, r]).copy()
        x, log = esp.gmres(A, np.ascontiguousarray(B[:, r]), Pl=P, x=x0, log=True, **kw)
        out.append((np.array(x), history_of(log), log["iters"], log["mvps"], log["reorth"], log["isconverged"]))
    return out


def many_call(esp, A, P, B, where, X0=None, **kw):
    """one call on host arrays or tensors -> (X as a NumPy array, logs)"""
    if where == "host":
        x = None if X0 is None else np.asfortranarray(X0).copy(order="F")
        X, logs = esp.gmres(A, np.asfortranarray(B), Pl=P, x=x, log=True, **kw)
        assert isinstance(X, np.ndarray) and X.flags.f_contiguous
        if x is not None:
            assert X is x
        return X, logs
    x = None if X0 is None else to_device(X0)
    X, logs = esp.gmres(A, to_device(B), Pl=P, x=x, log=True, **kw)
    assert X.is_cuda and (X.shape[0] <= 1 or X.stride(0) == 1)
    if x is not None:
        assert X is x
    return to_host(X), logs


def assert_columns(X, logs, want, what):
    """`want`: (x, history, iters, mvps, reorth, isconverged) per column"""
    assert X.shape[1] == len(logs) == len(want), what
    for r, (wx, wh, wit, wmv, wre, wconv) in enumerate(want):
        log = logs[r]
        assert sorted(log) == KEYS, what
        assert log["iters"] == wit and len(log["resnorm"]) == wit, (what, r, "iters", log["iters"], wit)
        assert log["mvps"] == wmv and log["reorth"] == wre and log["isconverged"] == wconv, (what, r, log, wmv, wre, wconv)
        assert same_bits(history_of(log), wh), (what, r, "history")
        assert same_bits(X[:, r], wx), (what, r, "x")


def both_places(esp, A, P, B, single, what, X0=None, **kw):
    for where in ("host", "torch"):
        X, logs = many_call(esp, A, P, B, where, X0=X0, **kw)
        assert_columns(X, logs, single, (what, where))


# ---- 1. against the model and the single call -------------------------------------------------------------------------------------------
_MATRICES = {}
_REFS = {}


def matrix(esp, name):
    if name not in _MATRICES:
        A = esp.fdrand(20, 20, 1) if name == "fdrand" else convdiff(esp, 2.0)
        B = np.asfortranarray(np.random.default_rng(len(name)).standard_normal((A.n, KMAX)))
        B.setflags(write=False)
        _MATRICES[name] = (A, host_arrays(A), B)
    return _MATRICES[name]


def references(model, orc, esp, kind, orth, name):
    """the model's and the single call's columns: made once per (kind, orth, matrix), never changed"""
    key = (kind, orth, name)
    if key not in _REFS:
        A, arrays, B = matrix(esp, name)
        M = model.precon(kind, arrays, orc)
        want = [tuple(model.gmres(M, arrays, B[:, r], restart=20, orth_meth=orth)) for r in range(KMAX)]
        P = PRECONS[kind](esp, A)
        try:
            single = single_calls(esp, A, P, B, restart=20, orth_meth=orth)
        finally:
            close(P)
        _REFS[key] = (want, single)
    return _REFS[key]


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", ["fdrand", "convdiff"])
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("kind", ["identity", "jacobi", "ilu0", "iluam"])
def test_against_the_model_and_the_single_call(esp, orc, model, kind, orth, name, where):
    assert esp._lib.ESP_MANY_CHUNK == MC                   # (KS straddles it)
    A, arrays, B = matrix(esp, name)
    want, single = references(model, orc, esp, kind, orth, name)
    P = PRECONS[kind](esp, A)
    try:
        for k in KS:
            X, logs = many_call(esp, A, P, B[:, :k], where, restart=20, orth_meth=orth)
            assert X.shape == (A.n, k)
            assert_columns(X, logs, want[:k], (kind, orth, name, k, where, "model"))
            assert_columns(X, logs, single[:k], (kind, orth, name, k, where, "single"))
    finally:
        close(P)


# ---- 2. columns that stop at different times in one chunk --------------------------------------------------------------------------------
CAP = 150


@pytest.mark.parametrize("restart", [5, 20])
@pytest.mark.parametrize("orth", ["mgs", "dgks"])
@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_columns_that_stop_at_different_times(esp, model, kind, orth, restart):
    A = convdiff(esp, 2.0)
    arrays = host_arrays(A)
    cols = staggered_columns(A, lambda v: model.mul(arrays, v))
    P = PRECONS[kind](esp, A)
    try:
        names = sorted(cols)
        Ball = np.stack([cols[c] for c in names], axis=1)
        base = dict(reltol=0.0, abstol=1e-3, restart=restart, orth_meth=orth)
        # maxiter: two more than the slowest column that stops needs
        probe = dict(zip(names, single_calls(esp, A, P, Ball, maxiter=CAP, **base)))
        slowest = max(probe[c][2] for c in names if c != "never")
        assert all(probe[c][5] for c in names if c != "never") and slowest + 2 < CAP
        kw = dict(maxiter=slowest + 2, **base)
        single = dict(zip(names, single_calls(esp, A, P, Ball, **kw)))
        iters = {c: single[c][2] for c in names}
        print(kind, orth, restart, iters)
        assert iters["zero"] == 0 and iters["tiny"] == 0 and single["zero"][5] and single["tiny"][5]
        assert iters["never"] == kw["maxiter"] and not single["never"][5]
        assert len(set(iters.values())) >= 4                                   # the chunk really stops column by column
        stops = [iters[c] for c in names if c != "never" and iters[c] > 0]
        # The recipe's counts were worked out on the CPU model for Identity and Jacobi with mgs: only there does the test insist on a
        # stop inside a cycle and one at its end.  The other kinds and dgks are held to four distinct counts alone, so for them a stop
        # exactly at a cycle's end may not occur and that mechanism may go unexercised (the printed counts say which it was).
        if kind in ("identity", "jacobi") and orth == "mgs":
            assert any(i % restart != 0 for i in stops)                        # a stop in the middle of a cycle
            if restart == 5:
                assert any(i % restart == 0 for i in stops)                    # ... and one exactly at its end
        for order, seq in ORDERS.items():
            for k in (8, 9):                                                   # one chunk; a chunk and a lone column
                B = np.stack([cols[c] for c in seq[:k]], axis=1)
                both_places(esp, A, P, B, [single[c] for c in seq[:k]], (kind, orth, restart, order, k), **kw)
    finally:
        close(P)


# ---- 3. the DGKS predicate per column ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [5, 20])
def test_dgks_predicate_per_column(esp, model, restart):
    A = convdiff(esp, 50.0)
    arrays = host_arrays(A)
    n = A.n
    rng = np.random.default_rng(29)
    e = np.zeros(n)
    e[n // 3] = 1.0
    B = np.stack([1e-3 * model.mul(arrays, e), 1e-3 * rng.standard_normal(n), rng.standard_normal(n), model.mul(arrays, np.ones(n)), e,
                  1e3 * rng.standard_normal(n)], axis=1)
    kw = dict(restart=restart, orth_meth="dgks", reltol=0.0, abstol=1e-3, maxiter=80)
    single = single_calls(esp, A, None, B, **kw)
    print(restart, [(s[2], s[4]) for s in single])
    assert len({s[4] for s in single}) > 1                                     # the pass counts differ between the columns
    assert any(0 < s[4] < s[2] for s in single)                                # ... and some iterations of a column correct, others not
    both_places(esp, A, None, B, single, ("dgks", restart), **kw)
    B9 = np.concatenate([B, B[:, :3][:, ::-1]], axis=1)                        # a chunk and a lone column
    both_places(esp, A, None, B9, single + single[:3][::-1], ("dgks 9", restart), **kw)


# ---- 4. restart lengths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("restart", [1, 2, 5, 9, 17, 64])
def test_restart_lengths(esp, orth, restart):
    A = tridiagonal(esp, 513)
    B = np.asfortranarray(np.random.default_rng(restart).standard_normal((513, 9)))
    P = esp.JacobiPreconditioner(A)
    try:
        kw = dict(restart=restart, orth_meth=orth, maxiter=40)
        single = single_calls(esp, A, P, B, **kw)
        assert all(s[2] == 40 or s[5] for s in single)
        if restart == 64:
            assert all(s[5] and s[2] < restart for s in single)                # restart > iterations
        both_places(esp, A, P, B, single, (orth, restart), **kw)
        if restart >= 9:                                                       # a full cycle (every group of the batched dots) and two more
            kw = dict(restart=restart, orth_meth=orth, maxiter=restart + 2, reltol=0.0)
            single = single_calls(esp, A, P, B, **kw)
            assert all(s[2] == restart + 2 and s[3] == restart + 3 for s in single)
            X, logs = many_call(esp, A, P, B, "torch", **kw)
            assert_columns(X, logs, single, (orth, restart, "full cycle"))
    finally:
        close(P)


# ---- 5. the summation shape's edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orth", ["mgs", "dgks"])
@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 513, 65537])
def test_summation_shape_edges(esp, kind, orth, n):
    A = tridiagonal(esp, n)
    B = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 9)))
    if n == 1:
        B = np.asfortranarray([[(-1.0) ** r * 2.0 ** (r - 4) for r in range(9)]])   # (powers of two: V1 = +-1 exactly)
    P = PRECONS[kind](esp, A)
    try:
        kw = dict(orth_meth=orth, maxiter=7) if n == 65537 else dict(orth_meth=orth, maxiter=40)
        single = single_calls(esp, A, P, B, **kw)
        if n == 1:                                                             # the lucky breakdown in every column
            assert all(s[2] == 1 and s[5] and s[1][1] == 0.0 for s in single)
        elif n < 65537:
            assert all(s[5] for s in single)
        both_places(esp, A, P, B, single, (kind, orth, n), **kw)
    finally:
        close(P)


def test_no_rows_and_no_columns(esp):
    import torch
    A0 = esp.ExtendableSparseMatrix(0, 0)
    X, logs = esp.gmres(A0, np.empty((0, 3), order="F"), log=True)
    assert X.shape == (0, 3) and len(logs) == 3
    _, one = esp.gmres(A0, np.empty(0), log=True)                               # the single call says the same
    for log in logs + [one]:
        assert log["iters"] == 0 and log["mvps"] == 0 and log["reorth"] == 0 and log["isconverged"] and log["r0"] == 0.0
    A = tridiagonal(esp, 257)
    X, logs = esp.gmres(A, np.empty((257, 0), order="F"), log=True)
    assert X.shape == (257, 0) and logs == []
    T = esp.gmres(A, torch.empty((0, 257), dtype=torch.float64, device="cuda").t())
    assert tuple(T.shape) == (257, 0)


# ---- 6. staged and unstaged row slices in one matrix ---------------------------------------------------------------------------------------
def nonsymmetric_band(esp, half):
    """test_cg_many_gpu's band matrix with its strict lower triangle scaled by 0.5"""
    cp, rv, nz = host_arrays(band_matrix(esp, half=half))
    S = sp.csc_matrix((nz, rv - 1, cp - 1))
    return from_scipy(esp, sp.triu(S) + 0.5 * sp.tril(S, -1))


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("half", [5, 9])
def test_staged_and_unstaged_row_slices(esp, kind, half, symmetric):
    A = band_matrix(esp, half=half) if symmetric else nonsymmetric_band(esp, half)
    rng = np.random.default_rng(half)
    B = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    X0 = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))                  # A*x over both kinds of slices
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B)
        assert all(s[5] for s in single)
        both_places(esp, A, P, B, single, (kind, half, symmetric))
        single = single_calls(esp, A, P, B, X0=X0, orth_meth="cgs")
        X, logs = many_call(esp, A, P, B, "torch", X0=X0, orth_meth="cgs")
        assert_columns(X, logs, single, (kind, half, symmetric, "gmres!"))
    finally:
        close(P)


# ---- 7. ends ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orth", ["mgs", "dgks"])
@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("maxiter", [0, 3, 5, 6])
def test_maxiter_ends_every_column(esp, kind, orth, maxiter):
    restart = 5                                                                # maxiter: 0, inside a cycle, restart, restart + 1
    A = convdiff(esp, 2.0)
    rng = np.random.default_rng(5)
    B = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    B[:, 4] = 0.0
    X0 = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        kw = dict(restart=restart, orth_meth=orth, maxiter=maxiter, reltol=0.0)
        single = single_calls(esp, A, P, B, **kw)
        assert [s[2] for s in single] == [0 if r == 4 else maxiter for r in range(MC + 1)]
        both_places(esp, A, P, B, single, (kind, orth, maxiter), **kw)
        single = single_calls(esp, A, P, B, X0=X0, **kw)                        # from a start: maxiter = 0 touches no x
        assert all(s[2] == maxiter for s in single)
        both_places(esp, A, P, B, single, (kind, orth, maxiter, "gmres!"), X0=X0, **kw)
        if maxiter == 0:
            assert same_bits(many_call(esp, A, P, B, "torch", X0=X0, **kw)[0], X0)
    finally:
        close(P)


@pytest.mark.parametrize("orth", ORTHS)
def test_a_nan_column_runs_to_maxiter_beside_the_others(esp, orth):
    A = convdiff(esp, 2.0)
    B = np.asfortranarray(np.random.default_rng(6).standard_normal((A.n, MC)))
    B[7, 2] = np.nan
    P = esp.ILU0Preconditioner(A)
    try:
        kw = dict(restart=5, orth_meth=orth, maxiter=60)
        single = single_calls(esp, A, P, B, **kw)
        assert single[2][2] == 60 and not single[2][5] and all(s[5] and s[2] < 60 for r, s in enumerate(single) if r != 2)
        X, logs = many_call(esp, A, P, B, "torch", **kw)
        assert_columns(X, logs, single, ("nan column", orth))
        assert np.all(np.isfinite(np.delete(X, 2, axis=1)))
    finally:
        close(P)


@pytest.mark.parametrize("kind", FUSED)
def test_a_column_below_the_tolerance_from_a_start_stays_untouched(esp, model, kind):
    A = convdiff(esp, 2.0)
    arrays = host_arrays(A)
    rng = np.random.default_rng(61)
    X0 = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    B = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    for r in (0, 5, MC):
        B[:, r] = model.mul(arrays, X0[:, r])                                   # b - A*x = 0 exactly: below any tolerance
    P = PRECONS[kind](esp, A)
    try:
        kw = dict(abstol=1e-6)
        single = single_calls(esp, A, P, B, X0=X0, **kw)
        for r in (0, 5, MC):
            assert single[r][2] == 0 and single[r][3] == 1 and single[r][5] and same_bits(single[r][0], X0[:, r])
        assert all(s[2] > 0 for r, s in enumerate(single) if r not in (0, 5, MC))
        for where in ("host", "torch"):
            X, logs = many_call(esp, A, P, B, where, X0=X0, **kw)
            assert_columns(X, logs, single, (kind, where))
            assert same_bits(X[:, [0, 5, MC]], X0[:, [0, 5, MC]])
    finally:
        close(P)


# ---- 8. gmres! and caller-owned memory --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_inplace_from_a_random_start(esp, kind, where):
    A = convdiff(esp, 2.0, (20, 20, 1))
    rng = np.random.default_rng(31)
    B = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    X0 = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        for orth in ("mgs", "dgks"):
            single = single_calls(esp, A, P, B, X0=X0, restart=7, orth_meth=orth)
            assert all(s[3] == s[2] + 1 + (s[2] - 1) // 7 for s in single)      # one product more for the start, one per restart
            X, logs = many_call(esp, A, P, B, where, X0=X0, restart=7, orth_meth=orth)   # (asserts that the given X comes back)
            assert_columns(X, logs, single, (kind, where, orth))
        assert not same_bits(X, many_call(esp, A, P, B, where, restart=7, orth_meth="dgks")[0])   # the start was read
    finally:
        close(P)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_leading_dimensions_and_guard_bands(esp, kind, device):
    A = convdiff(esp, 2.0, (21, 13, 1))                                         # n = 273: odd, more than one workgroup
    n, k = A.n, MC + 1
    ld = n + 5
    rng = np.random.default_rng(41)
    B = np.asfortranarray(rng.standard_normal((n, k)))
    X0 = np.asfortranarray(rng.standard_normal((n, k)))
    P = PRECONS[kind](esp, A)
    try:
        for orth in ("mgs", "cgs"):
            single = single_calls(esp, A, P, B, X0=X0, orth_meth=orth)
            b, bwhole, bcheck = strided(B, ld, 1, device)
            x, xwhole, xcheck = strided(X0, ld, 3, device)
            snap = frozen(bwhole)
            got, logs = esp.gmres(A, b, Pl=P, x=x, orth_meth=orth, log=True)
            A.synchronize()
            assert got is x
            assert_columns(to_host(got), logs, single, (kind, device, orth))
            snap.check("B")
            assert pads_intact(bwhole, n, ld, k) and pads_intact(xwhole, n, ld, k)  # the rows between the columns: never written
            bcheck("B"), xcheck("X")
        single = single_calls(esp, A, P, B)                                     # from zeros, into a new result
        got, logs = esp.gmres(A, b, Pl=P, log=True)
        assert_columns(to_host(got), logs, single, (kind, device, "gmres"))
        snap.check("B"), bcheck("B")
    finally:
        close(P)


def test_c_ordered_host_b_gives_the_f_ordered_bits(esp):
    A = convdiff(esp, 2.0, (20, 20, 1))
    B = np.random.default_rng(43).standard_normal((A.n, MC + 1))                # C-ordered
    assert B.flags.c_contiguous and not B.flags.f_contiguous
    P = esp.ILU0Preconditioner(A)
    try:
        keep = B.copy()
        X, logs = esp.gmres(A, B, Pl=P, log=True)
        XF, logsF = esp.gmres(A, np.asfortranarray(B), Pl=P, log=True)
        assert X.flags.f_contiguous and same_bits(X, XF) and np.array_equal(bits(B), bits(keep))
        for a, b in zip(logs, logsF):
            assert a["iters"] == b["iters"] > 0 and same_bits(history_of(a), history_of(b))
    finally:
        close(P)


# ---- 9. every other kind ----------------------------------------------------------------------------------------------------------------------
def block_ranges(inner):
    """a BlockPreconditioner over two contiguous ranges: its identity path, where the solvers take the INNER preconditioner's fused
    branch (Jacobi: the product kernel with the diagonal applied; ILU0: the two row passes) and the inner object belongs to the
    derived block matrix's handle, not to A's"""
    def make(esp, A):
        n = A.n
        P = esp.BlockPreconditioner(A, [np.arange(1, n // 2 + 1), np.arange(n // 2 + 1, n + 1)], getattr(esp, inner))
        assert P.path == 0
        return P
    return make


OTHER = dict(PRECONS, block_ranges_jacobi=block_ranges("JacobiPreconditioner"), block_ranges_ilu0=block_ranges("ILU0Preconditioner"))


@pytest.mark.parametrize("kind", ["cholesky", "lu_panels", "lu_columns", "iluk1", "ilut", "amg", "rsamg", "spai_sym", "block", "colored",
                                  "block_ranges_jacobi", "block_ranges_ilu0"])
def test_every_other_kind(esp, kind):
    A = esp.fdrand(10, 10, 10) if kind in ("cholesky", "amg", "spai_sym") else convdiff(esp, 2.0)
    B = np.asfortranarray(np.random.default_rng(47).standard_normal((A.n, MC + 1)))
    B[:, 3] *= 1e-9                                                             # stops early under the absolute tolerance
    P = OTHER[kind](esp, A)
    try:
        for orth in (ORTHS if kind.startswith("block_ranges") else ["mgs"]):    # (with and without the product's dot)
            kw = dict(abstol=1e-7, maxiter=25, restart=6, orth_meth=orth)
            single = single_calls(esp, A, P, B, **kw)
            print(kind, orth, [s[2] for s in single])
            both_places(esp, A, P, B, single, (kind, orth), **kw)
    finally:
        close(P)


def test_block_ranges_jacobi_is_jacobi_of_the_whole_matrix(esp):
    """the blocks of contiguous ranges keep A's diagonal, so this Block-of-Jacobi is plain Jacobi: the many-column product must
    multiply by A itself (not by the block matrix), and every column has the plain Jacobi solve's bits"""
    A = convdiff(esp, 2.0)
    B = np.asfortranarray(np.random.default_rng(48).standard_normal((A.n, MC + 1)))
    J = esp.JacobiPreconditioner(A)
    P = block_ranges("JacobiPreconditioner")(esp, A)
    try:
        kw = dict(restart=6, maxiter=25)
        plain = single_calls(esp, A, J, B, **kw)
        assert all(s[2] > 3 for s in plain)
        both_places(esp, A, P, B, plain, "block of jacobi against jacobi", **kw)
    finally:
        close(P)
        close(J)


# ---- 10. reproducibility and updates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orth", ["mgs", "dgks"])
@pytest.mark.parametrize("kind", FUSED + ["lu_panels"])
def test_reproducible_and_follows_updates(esp, kind, orth):
    A = convdiff(esp, 2.0)
    B = np.asfortranarray(np.random.default_rng(53).standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        kw = dict(restart=8, orth_meth=orth, maxiter=60)
        X1, logs1 = many_call(esp, A, P, B, "torch", **kw)
        X2, logs2 = many_call(esp, A, P, B, "torch", **kw)
        assert same_bits(X1, X2)
        for a, b in zip(logs1, logs2):
            assert a["iters"] == b["iters"] and a["reorth"] == b["reorth"] and same_bits(history_of(a), history_of(b))
        csc = A.sparse()
        csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
        A._push_edits()
        if P is not None:
            P.update()
        single = single_calls(esp, A, P, B, **kw)
        X3, logs3 = many_call(esp, A, P, B, "torch", **kw)
        assert_columns(X3, logs3, single, (kind, orth, "after update"))
        assert not same_bits(X3, X1)
    finally:
        close(P)


# ---- 11. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_through_ctypes(esp):
    import torch
    A = esp.fdrand(5, 4, 3)
    other = esp.fdrand(5, 4, 3)
    n = A.n
    lib, h = A._d.lib, A._d.h
    P, Q = esp.ILU0Preconditioner(A), esp.ILU0Preconditioner(other)
    try:
        b = torch.ones(4 * n, dtype=torch.float64, device="cuda")
        x = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
        its, mvs, re = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
        conv = (C.c_int32 * 4)()

        def call(p, B, ldb, X, ldx, k, maxiter=60, restart=20, orth=0):
            return lib.esp_gmres_many(h, p, B, ldb, X, ldx, k, 1, 1, restart, orth, maxiter, 0.0, RELTOL, None, its, mvs, re, conv)

        p = P._live()
        assert call(p, dev_ptr(b), n, dev_ptr(x), n, 0) == ESP_OK
        assert call(p, None, n, None, n, 0) == ESP_OK                            # nothing to read or write
        assert call(p, dev_ptr(b), n, dev_ptr(x), n, -1) == ESP_ERR_INVALID
        assert "k = -1" in lib.esp_last_error(h).decode()
        assert call(p, dev_ptr(b), n - 1, dev_ptr(x), n, 2) == ESP_ERR_INVALID
        assert "ldb = %d" % (n - 1) in lib.esp_last_error(h).decode()
        assert call(p, dev_ptr(b), n, dev_ptr(x), n - 1, 2) == ESP_ERR_INVALID
        assert "ldx = %d" % (n - 1) in lib.esp_last_error(h).decode()
        assert call(p, None, n, dev_ptr(x), n, 2) == ESP_ERR_INVALID
        assert call(p, dev_ptr(b), n, None, n, 2) == ESP_ERR_INVALID
        assert call(p, dev_ptr(b), n, dev_ptr(x), n, 2, maxiter=-1) == ESP_ERR_INVALID
        for restart in (0, 65, -1):                                              # what esp_gmres refuses, for every k
            for k in (0, 1, 2):
                assert call(p, dev_ptr(b), n, dev_ptr(x), n, k, restart=restart) == ESP_ERR_INVALID
        for orth in (3, -1):
            assert call(p, dev_ptr(b), n, dev_ptr(x), n, 2, orth=orth) == ESP_ERR_INVALID
        # overlaps: the same array, shifted by a column, by one element from behind
        assert call(p, dev_ptr(b), n, dev_ptr(b), n, 3) == ESP_ERR_INVALID
        assert "overlap" in lib.esp_last_error(h).decode()
        assert call(p, dev_ptr(b), n, dev_ptr(b, n), n, 3) == ESP_ERR_INVALID
        assert call(p, dev_ptr(b, 3 * n - 1), n, dev_ptr(b), n, 3) == ESP_ERR_INVALID
        assert call(Q._live(), dev_ptr(b), n, dev_ptr(x), n, 2) == ESP_ERR_INVALID
        assert "another matrix" in lib.esp_last_error(h).decode()
        assert lib.esp_gmres_many(None, p, dev_ptr(b), n, dev_ptr(x), n, 2, 1, 1, 20, 0, 60, 0.0, RELTOL, None, its, mvs, re,
                                  conv) == ESP_ERR_INVALID
        assert bool((b == 1.0).all()) and not bool(x.any())                      # refused before anything was launched
        assert call(p, dev_ptr(b), n, dev_ptr(b, 3 * n), n, 1) == ESP_OK         # touching ranges do not overlap (k = 1: esp_gmres)
        b.fill_(1.0)
        for orth in (0, 1, 2):
            x.zero_()
            assert call(p, dev_ptr(b), n, dev_ptr(x), n, 3, orth=orth) == ESP_OK
            assert list(its)[:3] == [its[0]] * 3 and its[0] > 0 and list(conv)[:3] == [1, 1, 1] and list(mvs)[:3] == [its[0]] * 3
        assert lib.esp_gmres_many(h, p, dev_ptr(b), n, dev_ptr(x), n, 3, 1, 1, 20, 2, 60, 0.0, RELTOL, None, None, None, None,
                                  None) == ESP_OK                                # every out pointer is optional
        A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.25, 0.25])                   # a pattern change without update()
        A.flush()
        for k in (0, 1, 2, 3):
            assert call(p, dev_ptr(b), n, dev_ptr(x), n, k) == ESP_ERR_STATE
        with pytest.raises(esp.EspError) as e:
            esp.gmres(A, np.ones((n, 2), order="F"), Pl=P)
        assert e.value.code == ESP_ERR_STATE
    finally:
        P.close()
        Q.close()


def test_python_refusals(esp):
    import torch
    A = esp.fdrand(5, 4, 3)
    other = esp.fdrand(5, 4, 3)
    n, k = A.n, 3
    P, Q = esp.ILU0Preconditioner(A), esp.ILU0Preconditioner(other)
    try:
        B = np.asfortranarray(np.random.default_rng(3).standard_normal((n, k)))
        X = np.asfortranarray(np.random.default_rng(4).standard_normal((n, k)))
        keepB, keepX = B.copy(), X.copy()
        with pytest.raises(ValueError):
            esp.gmres(A, B, Pl=Q)                                               # Pl of another matrix
        with pytest.raises(ValueError):
            esp.gmres(A, B, Pl=P, x=to_device(X))                               # B on the host with X on the device
        with pytest.raises(ValueError):
            esp.gmres(A, to_device(B), Pl=P, x=X)                               # ... and the other way round
        with pytest.raises(ValueError, match="DimensionMismatch"):
            esp.gmres(A, B, Pl=P, x=np.zeros((n, k + 1), order="F"))
        with pytest.raises(ValueError):
            esp.gmres(A, B, Pl=P, x=np.zeros((n, k)))                           # a C-ordered x cannot be updated in place
        with pytest.raises(ValueError):
            esp.gmres(A, B, Pl=P, x=np.zeros(n))                                # a 1-D x with a 2-D b
        with pytest.raises(ValueError):
            esp.gmres(A, B[:, 0].copy(), Pl=P, x=X)                             # ... and a 1-D b with a 2-D x
        with pytest.raises(ValueError, match="maxiter < 0"):
            esp.gmres(A, B, Pl=P, x=X, maxiter=-1)
        with pytest.raises(ValueError):
            esp.gmres(A, B, Pl=P, orth_meth="householder")
        for restart in (0, 65):
            with pytest.raises(esp.EspError) as e:
                esp.gmres(A, B, Pl=P, x=X, restart=restart)
            assert e.value.code == ESP_ERR_INVALID
        for bad in (np.zeros((n + 1, k)), np.zeros((n, k, 2)), np.zeros((n, k), np.float32),
                    torch.zeros((n, k), dtype=torch.float64, device="cuda")):    # row-major tensor: stride(0) != 1
            with pytest.raises(ValueError, match="DimensionMismatch"):
                esp.gmres(A, bad, Pl=P)
        assert np.array_equal(bits(B), bits(keepB)) and np.array_equal(bits(X), bits(keepX))
        assert same_bits(esp.gmres(A, B[:, 0].copy(), Pl=P), esp.gmres(A, B, Pl=P)[:, 0])   # and both forms still work
    finally:
        P.close()
        Q.close()
