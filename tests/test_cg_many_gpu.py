"""GPU: conjugate gradients for several right-hand sides -- cg(A, B) with an (n, k) B (include/esparse_hip.h, esp_cg_many; DESIGN.md
5u).  The contract is one sentence: for every column r, x[:, r], the whole residual history of r, its iteration count and its
converged flag are bit for bit what the single call gives for column r alone -- whatever the other columns of the chunk hold and
whenever they stop.  Where tests/cg_model.c has the kind (Identity, Jacobi, ILU0, ILUAM) the columns are held to the model as well.

The constants and the sizes that straddle them:
  MC = 8        columns of a chunk (ESP_MANY_CHUNK).  Column counts k: 2, 7, 8, 9, 17 (a narrow chunk, one short of a chunk, a full
                chunk, a chunk and one column, two chunks and one).
  KT = 256      elements of a chunk of the summation shape = rows of a workgroup: n in 1, 255, 256, 257, 513, and 65537, where the
                second level has two groups (nb1 = 2).
  KCAP = 2048   entries of a row slice a workgroup stages in LDS: a band matrix whose first 256 rows hold more, the rest fewer."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from cg_modellib import RELTOL, Model
from device_views import frozen, guarded
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_OK, ESP_ERR_INVALID, ESP_ERR_STATE = 0, -1, -6
MC = 8
KS = [2, 7, 8, 9, 17]
KMAX = max(KS)
PAD_BITS = 0x7FF8DEADBEEF5A5B    # device_views' float64 canary


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("cg_many_model"))


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


def from_scipy(esp, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    m, n = S.shape
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(m, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def tridiagonal(esp, n):
    return from_scipy(esp, sp.diags([-np.ones(max(n - 1, 0)), 4.0 * np.ones(n), -np.ones(max(n - 1, 0))], [-1, 0, 1], format="csc"))


def band_matrix(esp, n=700, wide=300, half=5):
    """symmetric, diagonally dominant: the entries (i, j) with 0 < |i - j| <= half and min(i, j) < wide, and the tridiagonal ones.
    half = 5: the first `wide` rows hold 11 entries each (but the first five), 256 of them more than KCAP = 2048; half = 9: 19
    entries each, so that the strictly lower and upper parts ILU0 walks hold more than KCAP per 256 rows as well"""
    rng = np.random.default_rng(17)
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in range(i + 1, min(i + half, n - 1) + 1):
            if j == i + 1 or i < wide:
                v = -(0.5 + 0.5 * rng.random())
                rows += [i, j]
                cols += [j, i]
                vals += [v, v]
    S = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    S = S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)
    if half == 5:
        counts = np.diff(sp.csr_matrix(S).indptr)
        assert np.all(counts[5:wide] == 11) and counts[:256].sum() > 2048 and counts[256:512].sum() <= 2048
    return from_scipy(esp, S)


def to_device(X):
    """an (n, k) array as a CUDA tensor with stride (1, n)"""
    import torch
    X = np.asarray(X, np.float64)
    return torch.from_numpy(np.ascontiguousarray(X.T).copy()).cuda().t()


def to_host(T):
    return T.cpu().numpy() if hasattr(T, "cpu") else np.asarray(T)


def interleaved(n):
    return [range(1, n + 1, 2), range(2, n + 1, 2)]


PRECONS = {
    "identity": lambda esp, A: None,
    "jacobi": lambda esp, A: esp.JacobiPreconditioner(A),
    "ilu0": lambda esp, A: esp.ILU0Preconditioner(A),
    "iluam": lambda esp, A: esp.ILUAMPreconditioner(A),
    "cholesky": lambda esp, A: esp.CholeskyFactorization(A, 16),
    "lu_panels": lambda esp, A: esp.LUFactorization(A, 16, form="panels"),
    "lu_columns": lambda esp, A: esp.LUFactorization(A, 16, form="columns"),
    "iluk1": lambda esp, A: esp.ILUKPreconditioner(A, 1),
    "ilut": lambda esp, A: esp.ILUTPreconditioner(A),
    "amg": lambda esp, A: esp.AMGPreconditioner(A, max_coarse=16),
    "rsamg": lambda esp, A: esp.RS_AMGPreconditioner(A, max_coarse=16),
    "spai_sym": lambda esp, A: esp.SPAIPreconditioner(A, 1, True),
    "block": lambda esp, A: esp.BlockPreconditioner(A, interleaved(A.n), esp.ILU0Preconditioner),
    "colored": lambda esp, A: esp.ColoredPreconditioner(A),
}
FUSED = ["identity", "jacobi", "ilu0"]


def close(P):
    if P is not None:
        P.close()


def single_calls(esp, A, P, B, X0=None, **kw):
    """the single call on every column: [(x, history, iters, isconverged)]"""
    out = []
    for r in range(B.shape[1]):
        x0 = None if X0 is None else np.ascontiguousarray(X0[:, r]).copy()
        x, log = esp.cg(A, np.ascontiguousarray(B[:, r]), Pl=P, x=x0, log=True, **kw)
        out.append((np.array(x), history_of(log), log["iters"], log["isconverged"]))
    return out


def many_call(esp, A, P, B, where, X0=None, **kw):
    """one call on host arrays or tensors -> (X as a NumPy array, logs)"""
    if where == "host":
        x = None if X0 is None else np.asfortranarray(X0).copy(order="F")
        X, logs = esp.cg(A, np.asfortranarray(B), Pl=P, x=x, log=True, **kw)
        assert isinstance(X, np.ndarray) and X.flags.f_contiguous
        if x is not None:
            assert X is x
        return X, logs
    x = None if X0 is None else to_device(X0)
    X, logs = esp.cg(A, to_device(B), Pl=P, x=x, log=True, **kw)
    assert X.is_cuda and (X.shape[0] <= 1 or X.stride(0) == 1)
    if x is not None:
        assert X is x
    return to_host(X), logs


def assert_columns(X, logs, want, what):
    """`want`: (x, history, iters, isconverged) per column"""
    assert X.shape[1] == len(logs) == len(want), what
    for r, (wx, wh, wit, wconv) in enumerate(want):
        log = logs[r]
        assert sorted(log) == ["isconverged", "iters", "r0", "resnorm"], what
        assert log["iters"] == wit and log["isconverged"] == wconv and len(log["resnorm"]) == wit, (what, r, log["iters"], wit)
        assert same_bits(history_of(log), wh), (what, r, "history")
        assert same_bits(X[:, r], wx), (what, r, "x")


# ---- 1. against the model and the single call -------------------------------------------------------------------------------------------
_REFS = {}


def references(model, orc, esp, kind, dims):
    """the matrix, KMAX right-hand sides, the model's and the single call's columns: made once per (kind, matrix), never changed"""
    if (kind, dims) not in _REFS:
        A = esp.fdrand(*dims)
        arrays = host_arrays(A)
        B = np.asfortranarray(np.random.default_rng(sum(dims)).standard_normal((A.n, KMAX)))
        B.setflags(write=False)
        M = model.precon(kind, arrays, orc)
        want = [model.cg(M, arrays, B[:, r]) for r in range(KMAX)]
        P = PRECONS[kind](esp, A)
        try:
            single = single_calls(esp, A, P, B)
        finally:
            close(P)
        _REFS[(kind, dims)] = (A, B, want, single)
    return _REFS[(kind, dims)]


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("dims", [(20, 20, 1), (10, 10, 10)])
@pytest.mark.parametrize("kind", ["identity", "jacobi", "ilu0", "iluam"])
def test_against_the_model_and_the_single_call(esp, orc, model, kind, dims, where):
    assert esp._lib.ESP_MANY_CHUNK == MC                   # (KS straddles it)
    A, B, want, single = references(model, orc, esp, kind, dims)
    for r in range(KMAX):                                   # the yardstick itself: the single call is the model's
        assert single[r][2] == want[r][2] and single[r][3] == want[r][3]
        assert same_bits(single[r][1], want[r][1]) and same_bits(single[r][0], want[r][0])
    P = PRECONS[kind](esp, A)
    try:
        for k in KS:
            X, logs = many_call(esp, A, P, B[:, :k], where)
            assert X.shape == (A.n, k)
            assert_columns(X, logs, want[:k], (kind, dims, k, where, "model"))
            assert_columns(X, logs, single[:k], (kind, dims, k, where, "single"))
    finally:
        close(P)


# ---- 2. columns that stop at different times in one chunk --------------------------------------------------------------------------------
def staggered_columns(A, model_mul):
    """name -> column.  With reltol = 0 and abstol = 1e-3 the scale of a column decides when it stops: `zero` at once, `tiny` below
    the tolerance from the start, `axis` (A e_j scaled) and `small` (a reduction by 30 or so) early, the random ones later, `never`
    (scaled by 1e30) not within any maxiter: its tolerance asks for a reduction no double holds"""
    n = A.n
    rng = np.random.default_rng(23)
    e = np.zeros(n)
    e[n // 3] = 1.0
    return {"zero": np.zeros(n), "tiny": 1e-12 * rng.standard_normal(n), "axis": 1e-3 * model_mul(e),
            "small": 1e-3 * rng.standard_normal(n), "rand1": rng.standard_normal(n), "rand2": 1e3 * rng.standard_normal(n),
            "rand3": rng.standard_normal(n), "never": 1e30 * rng.standard_normal(n), "rand4": 10.0 * rng.standard_normal(n)}


CAP = 150
ORDERS = {
    "early_first": ["zero", "tiny", "axis", "small", "rand1", "rand2", "never", "rand3", "rand4"],
    "early_last": ["rand1", "never", "rand2", "rand3", "small", "axis", "tiny", "zero", "rand4"],
    "early_middle": ["rand1", "rand2", "zero", "axis", "tiny", "never", "small", "rand3", "rand4"],
}


@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_columns_that_stop_at_different_times(esp, model, kind):
    A = esp.fdrand(10, 10, 10)
    arrays = host_arrays(A)
    cols = staggered_columns(A, lambda v: model.mul(arrays, v))
    P = PRECONS[kind](esp, A)
    try:
        names = sorted(cols)
        Ball = np.stack([cols[c] for c in names], axis=1)
        # maxiter: two more than the slowest column that stops needs (the recurrence's residual of `never` would get there in the end)
        probe = dict(zip(names, single_calls(esp, A, P, Ball, reltol=0.0, abstol=1e-3, maxiter=CAP)))
        assert probe["rand2"][3] and probe["rand2"][2] + 2 < probe["never"][2]
        kw = dict(reltol=0.0, abstol=1e-3, maxiter=probe["rand2"][2] + 2)
        single = dict(zip(names, single_calls(esp, A, P, Ball, **kw)))
        iters = {c: single[c][2] for c in names}
        print(kind, iters)
        assert iters["zero"] == 0 and iters["tiny"] == 0 and single["zero"][3] and single["tiny"][3]
        assert iters["never"] == kw["maxiter"] and not single["never"][3]
        assert len(set(iters.values())) >= 4                                   # the chunk really stops column by column
        assert 0 < iters["small"] < iters["rand2"] < kw["maxiter"] and single["rand2"][3]
        for order, seq in ORDERS.items():
            for k in (8, 9):                                                   # one chunk; a chunk and a lone column
                B = np.stack([cols[c] for c in seq[:k]], axis=1)
                for where in ("host", "torch"):
                    X, logs = many_call(esp, A, P, B, where, **kw)
                    assert_columns(X, logs, [single[c] for c in seq[:k]], (kind, order, k, where))
    finally:
        close(P)


@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("maxiter", [0, 3])
def test_maxiter_ends_every_column(esp, kind, maxiter):
    A = esp.fdrand(10, 10, 10)
    B = np.asfortranarray(np.random.default_rng(5).standard_normal((A.n, MC + 1)))
    B[:, 4] = 0.0
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B, maxiter=maxiter)
        assert [s[2] for s in single] == [0 if r == 4 else maxiter for r in range(MC + 1)]
        for where in ("host", "torch"):
            X, logs = many_call(esp, A, P, B, where, maxiter=maxiter)
            assert_columns(X, logs, single, (kind, maxiter, where))
    finally:
        close(P)


def test_a_nan_column_runs_to_maxiter_beside_the_others(esp):
    A = esp.fdrand(10, 10, 10)
    B = np.asfortranarray(np.random.default_rng(6).standard_normal((A.n, MC)))
    B[7, 2] = np.nan
    P = esp.ILU0Preconditioner(A)
    try:
        single = single_calls(esp, A, P, B, maxiter=100)
        assert single[2][2] == 100 and not single[2][3] and all(s[3] and s[2] < 100 for r, s in enumerate(single) if r != 2)
        X, logs = many_call(esp, A, P, B, "torch", maxiter=100)
        assert_columns(X, logs, single, "nan column")
        assert np.all(np.isfinite(np.delete(X, 2, axis=1)))
    finally:
        close(P)


# ---- 3. the summation shape's edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 65537])
def test_summation_shape_edges(esp, kind, n):
    A = tridiagonal(esp, n)
    B = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 9)))
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B, maxiter=40)
        assert all(s[3] for s in single)
        for k in (3, 9):
            for where in ("host", "torch"):
                X, logs = many_call(esp, A, P, B[:, :k], where, maxiter=40)
                assert_columns(X, logs, single[:k], (kind, n, k, where))
    finally:
        close(P)


def test_no_rows(esp):
    import torch
    A0 = esp.ExtendableSparseMatrix(0, 0)
    X, logs = esp.cg(A0, np.empty((0, 3), order="F"), log=True)
    assert X.shape == (0, 3) and len(logs) == 3
    _, one = esp.cg(A0, np.empty(0), log=True)                                  # the single call says the same
    for log in logs + [one]:
        assert log["iters"] == 0 and log["isconverged"] and log["r0"] == 0.0 and len(log["resnorm"]) == 0
    T, logs = esp.cg(A0, torch.empty((3, 0), dtype=torch.float64, device="cuda").t(), log=True)
    assert tuple(T.shape) == (0, 3) and len(logs) == 3 and all(l["isconverged"] and l["iters"] == 0 for l in logs)
    assert esp.cg(A0, np.empty((0, 0), order="F")).shape == (0, 0)


@pytest.mark.parametrize("kind", FUSED)
def test_no_columns(esp, kind):
    import torch
    A = tridiagonal(esp, 257)
    P = PRECONS[kind](esp, A)
    try:
        X, logs = esp.cg(A, np.empty((257, 0), order="F"), Pl=P, log=True)
        assert X.shape == (257, 0) and logs == []
        T = esp.cg(A, torch.empty((0, 257), dtype=torch.float64, device="cuda").t(), Pl=P)
        assert tuple(T.shape) == (257, 0)
    finally:
        close(P)


# ---- 4. staged and unstaged row slices in one matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("half", [5, 9])
def test_staged_and_unstaged_row_slices(esp, kind, half):
    A = band_matrix(esp, half=half)
    B = np.asfortranarray(np.random.default_rng(half).standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B)
        assert all(s[3] for s in single)
        for where in ("host", "torch"):
            X, logs = many_call(esp, A, P, B, where)
            assert_columns(X, logs, single, (kind, half, where))
        X0 = np.asfortranarray(np.random.default_rng(half + 1).standard_normal((A.n, MC + 1)))   # c = A*x over both slices
        single = single_calls(esp, A, P, B, X0=X0)
        X, logs = many_call(esp, A, P, B, "torch", X0=X0)
        assert_columns(X, logs, single, (kind, half, "cg!"))
    finally:
        close(P)


# ---- 5. cg! -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_cg_inplace_from_a_random_start(esp, kind, where):
    A = esp.fdrand(20, 20, 1)
    rng = np.random.default_rng(31)
    B = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    X0 = np.asfortranarray(rng.standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B, X0=X0)
        X, logs = many_call(esp, A, P, B, where, X0=X0)                         # (asserts that the given X is what comes back)
        assert_columns(X, logs, single, (kind, where))
        assert not same_bits(X, many_call(esp, A, P, B, where)[0])              # the start was read
    finally:
        close(P)


# ---- 6. caller-owned memory -------------------------------------------------------------------------------------------------------------------
def strided(values, ld, lead, device):
    """(view, whole, check): the (n, k) `values` as a column-major view with leading dimension ld at element offset `lead` of a
    guarded buffer; the ld - n pad rows between the columns hold the canary NaN and belong to `whole` (ld * k elements)"""
    import torch
    n, k = values.shape
    flat = np.empty(ld * k)
    flat.view(np.uint64)[:] = PAD_BITS
    for r in range(k):
        flat[r * ld:r * ld + n] = values[:, r]
    g = guarded(torch.from_numpy(flat).cuda() if device else flat, lead)
    if device:
        view = torch.as_strided(g.view, (n, k), (1, ld))
    else:
        view = np.lib.stride_tricks.as_strided(g.view, (n, k), (8, 8 * ld))
    return view, g.view, g.check


def pads_intact(whole, n, ld, k):
    w = to_host(whole).view(np.uint64).reshape(k, ld)
    return bool(np.all(w[:, n:] == PAD_BITS))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kind", FUSED + ["iluam"])
def test_leading_dimensions_and_guard_bands(esp, kind, device):
    A = esp.fdrand(21, 13, 1)                                                   # n = 273: odd, more than one workgroup
    n, k = A.n, MC + 1
    ld = n + 5
    rng = np.random.default_rng(41)
    B = np.asfortranarray(rng.standard_normal((n, k)))
    X0 = np.asfortranarray(rng.standard_normal((n, k)))
    P = PRECONS[kind](esp, A)
    try:
        single = single_calls(esp, A, P, B, X0=X0)
        b, bwhole, bcheck = strided(B, ld, 1, device)
        x, xwhole, xcheck = strided(X0, ld, 3, device)
        snap = frozen(bwhole)
        got, logs = esp.cg(A, b, Pl=P, x=x, log=True)
        A.synchronize()
        assert got is x
        assert_columns(to_host(got), logs, single, (kind, device))
        snap.check("B")
        assert pads_intact(bwhole, n, ld, k) and pads_intact(xwhole, n, ld, k)  # the rows between the columns: never written
        bcheck("B"), xcheck("X")
        # from zeros, into a new result
        single = single_calls(esp, A, P, B)
        got, logs = esp.cg(A, b, Pl=P, log=True)
        assert_columns(to_host(got), logs, single, (kind, device, "cg"))
        snap.check("B"), bcheck("B")
    finally:
        close(P)


def test_c_ordered_host_b_gives_the_f_ordered_bits(esp):
    A = esp.fdrand(20, 20, 1)
    B = np.random.default_rng(43).standard_normal((A.n, MC + 1))                # C-ordered
    assert B.flags.c_contiguous and not B.flags.f_contiguous
    P = esp.ILU0Preconditioner(A)
    try:
        keep = B.copy()
        X, logs = esp.cg(A, B, Pl=P, log=True)
        XF, logsF = esp.cg(A, np.asfortranarray(B), Pl=P, log=True)
        assert X.flags.f_contiguous and same_bits(X, XF) and np.array_equal(bits(B), bits(keep))
        for a, b in zip(logs, logsF):
            assert a["iters"] == b["iters"] and same_bits(history_of(a), history_of(b))
    finally:
        close(P)


# ---- 7. every other kind ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cholesky", "lu_panels", "lu_columns", "iluk1", "ilut", "amg", "rsamg", "spai_sym", "block", "colored"])
def test_every_other_kind(esp, kind):
    A = esp.fdrand(8, 8, 8)
    B = np.asfortranarray(np.random.default_rng(47).standard_normal((A.n, MC + 1)))
    B[:, 3] *= 1e-9                                                             # stops early under the absolute tolerance
    P = PRECONS[kind](esp, A)
    try:
        kw = dict(abstol=1e-7, maxiter=25)
        single = single_calls(esp, A, P, B, **kw)
        print(kind, [s[2] for s in single])
        for where in ("host", "torch"):
            X, logs = many_call(esp, A, P, B, where, **kw)
            assert_columns(X, logs, single, (kind, where))
    finally:
        close(P)


# ---- 8. reproducibility and updates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FUSED + ["cholesky"])
def test_reproducible_and_follows_updates(esp, kind):
    A = esp.fdrand(10, 10, 10)
    B = np.asfortranarray(np.random.default_rng(53).standard_normal((A.n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        X1, logs1 = many_call(esp, A, P, B, "torch")
        X2, logs2 = many_call(esp, A, P, B, "torch")
        assert same_bits(X1, X2)
        for a, b in zip(logs1, logs2):
            assert a["iters"] == b["iters"] and same_bits(history_of(a), history_of(b))
        csc = A.sparse()
        csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))   # (symmetry is not needed for bits)
        A._push_edits()
        if P is not None:
            P.update()
        single = single_calls(esp, A, P, B, maxiter=60)
        X3, logs3 = many_call(esp, A, P, B, "torch", maxiter=60)
        assert_columns(X3, logs3, single, (kind, "after update"))
        assert not same_bits(X3, X1)
    finally:
        close(P)


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------------
def dev_ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 8 * offset)


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
        its = (C.c_int64 * 4)()
        conv = (C.c_int32 * 4)()

        def call(p, B, ldb, X, ldx, k, maxiter=60):
            return lib.esp_cg_many(h, p, B, ldb, X, ldx, k, 1, 1, maxiter, 0.0, RELTOL, None, its, conv)

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
        # overlaps: the same array, shifted by a column, by one element from behind
        assert call(p, dev_ptr(b), n, dev_ptr(b), n, 3) == ESP_ERR_INVALID
        assert "overlap" in lib.esp_last_error(h).decode()
        assert call(p, dev_ptr(b), n, dev_ptr(b, n), n, 3) == ESP_ERR_INVALID
        assert call(p, dev_ptr(b, 3 * n - 1), n, dev_ptr(b), n, 3) == ESP_ERR_INVALID
        assert call(Q._live(), dev_ptr(b), n, dev_ptr(x), n, 2) == ESP_ERR_INVALID
        assert "another matrix" in lib.esp_last_error(h).decode()
        assert lib.esp_cg_many(None, p, dev_ptr(b), n, dev_ptr(x), n, 2, 1, 1, 60, 0.0, RELTOL, None, its, conv) == ESP_ERR_INVALID
        assert bool((b == 1.0).all()) and not bool(x.any())                      # refused before anything was launched
        assert call(p, dev_ptr(b), n, dev_ptr(b, 3 * n), n, 1) == ESP_OK         # touching ranges do not overlap (k = 1: esp_cg)
        b.fill_(1.0)
        assert call(p, dev_ptr(b), n, dev_ptr(x), n, 3) == ESP_OK
        assert list(its)[:3] == [its[0]] * 3 and its[0] > 0 and list(conv)[:3] == [1, 1, 1]
        A.append(esp.ESP_UPDATE, [n, 1], [1, n], [0.25, 0.25])                   # a pattern change without update()
        A.flush()
        for k in (0, 1, 2, 3):
            assert call(p, dev_ptr(b), n, dev_ptr(x), n, k) == ESP_ERR_STATE
        with pytest.raises(esp.EspError) as e:
            esp.cg(A, np.ones((n, 2), order="F"), Pl=P)
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
            esp.cg(A, B, Pl=Q)                                                  # Pl of another matrix
        with pytest.raises(ValueError):
            esp.cg(A, B, Pl=P, x=to_device(X))                                  # NumPy B with a tensor x
        with pytest.raises(ValueError):
            esp.cg(A, to_device(B), Pl=P, x=X)                                  # ... and the other way round
        with pytest.raises(ValueError, match="DimensionMismatch"):
            esp.cg(A, B, Pl=P, x=np.zeros((n, k + 1), order="F"))
        with pytest.raises(ValueError):
            esp.cg(A, B, Pl=P, x=np.zeros((n, k)))                              # a C-ordered x cannot be updated in place
        with pytest.raises(ValueError, match="maxiter < 0"):
            esp.cg(A, B, Pl=P, x=X, maxiter=-1)
        with pytest.raises(ValueError):
            esp.cg(A, B[:, 0].copy(), Pl=P, x=X)                                # 1-D b with a 2-D x
        for bad in (np.zeros((n + 1, k)), np.zeros((n, k, 2)), np.zeros((n, k), np.float32),
                    torch.zeros((n, k), dtype=torch.float64, device="cuda")):    # row-major tensor: stride(0) != 1
            with pytest.raises(ValueError, match="DimensionMismatch"):
                esp.cg(A, bad, Pl=P)
        assert np.array_equal(bits(B), bits(keepB)) and np.array_equal(bits(X), bits(keepX))
        assert same_bits(esp.cg(A, B[:, 0].copy(), Pl=P), esp.cg(A, B, Pl=P)[:, 0])   # and both forms still work
    finally:
        P.close()
        Q.close()


# ---- 10. esp_precon_ldiv_many of Jacobi and ILU0 on the many-column kernels ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
@pytest.mark.parametrize("matrix", ["band5", "band9", "tri257"])
def test_ldiv_many_on_the_fused_kernels(esp, kind, matrix):
    A = tridiagonal(esp, 257) if matrix == "tri257" else band_matrix(esp, half=int(matrix[4:]))
    n = A.n
    V = np.asfortranarray(np.random.default_rng(59).standard_normal((n, MC + 1)))
    P = PRECONS[kind](esp, A)
    try:
        single = np.stack([P.ldiv(np.ascontiguousarray(V[:, r])) for r in range(MC + 1)], axis=1)
        for k in (2, MC, MC + 1):
            Vk = np.asfortranarray(V[:, :k])
            assert same_bits(P.ldiv(Vk), single[:, :k]), (kind, matrix, k, "host")
            H = Vk.copy(order="F")
            assert P.ldiv(H, out=H) is H and same_bits(H, single[:, :k]), (kind, matrix, k, "host in place")
            T = to_device(Vk)
            assert same_bits(to_host(P.ldiv(T)), single[:, :k]) and same_bits(to_host(T), Vk), (kind, matrix, k, "device")
            assert P.ldiv(T, out=T) is T and same_bits(to_host(T), single[:, :k]), (kind, matrix, k, "device in place")
            v, vwhole, vcheck = strided(Vk, n + 5, 1, True)                      # any leading dimension, an odd offset
            assert P.ldiv(v, out=v) is v
            A.synchronize()
            assert same_bits(to_host(v), single[:, :k]) and pads_intact(vwhole, n, n + 5, k)
            vcheck("V = U")
    finally:
        close(P)
