"""GPU: ILUAM's two triangular solves for a chunk of right-hand sides in ONE pass over the level schedules (iluam_solve_many,
DESIGN.md 5w), behind esp_precon_ldiv_many, esp_cg_many and esp_gmres_many for ILUAM and every kind that ends in it.  The contract is
5t's sentence: column r is bit for bit what the single-vector call gives for column r alone.  The columns are held to the CPU model
of tests/iluam_model.c as well (on the device's own factor), so the new kernels answer to the model and not only to their twin; and
esp_precon_many_stats tells that the one-pass form really ran, with one column's launch count.

The constants and the sizes that straddle them:
  MC = 8     columns of a chunk: k in 0, 1, 2, 7, 8, 9, 17.
  LT = 256   lanes of a workgroup = the most members the levels of one thin launch hold together; a wider level is a launch of its
             own over count * MC lanes.  Level widths 255, 256, 257; 100 + 100 + 56 (one thin launch) against 100 + 100 + 57 (two).
  LT / MC = 32  members a thin launch takes per pass: level widths 1, 31, 32, 33.
The matrices have PRESCRIBED level widths (layered): level l holds w[l] consecutive unknowns, each coupled to unknowns of level l - 1
alone, so the forward schedule has exactly the widths w and the backward one their reverse.  Every unknown of level l is coupled to
(q mod w[l-1]) and up to two more of level l - 1; where a level is narrower than the one before it, the unknowns of level l - 1 that
nobody chose are coupled to (r mod w[l]) -- without that they would have no successor and fall into the backward schedule's first
level -- so behind a narrowing an unknown can have more than three couplings (257 in [257, 1, 257])."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from device_views import guarded
from iluam_modellib import Model, level_schedules
from refmodel import bits

pytestmark = pytest.mark.gpu

MC, LT = 8, 256
KS = [0, 1, 2, 7, 8, 9, 17]
KMAX = max(KS)
PAD_BITS = 0x7FF8DEADBEEF5A5B    # device_views' float64 canary

WIDTHS = {
    "w1": [1], "w31": [31], "w32": [32], "w33": [33],
    "w255": [255], "w256": [256], "w257": [257],
    "one_thin": [100, 100, 56],
    "two_thin": [100, 100, 57],
    "wide_1_wide": [257, 1, 257],
    "chain300": [1] * 300,
    "mixed": [40] * 9 + [300] * 2 + [5] * 7,
}
CASES = sorted(WIDTHS) + ["fdrand987", "empty"]
FORMS = ["host_f", "host_c", "device", "inplace", "guarded"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("iluam_many_model"))


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def from_scipy(esp, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    m, n = S.shape
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(m, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def to_device(X):
    """an (n, k) array as a CUDA tensor with stride (1, n)"""
    import torch
    X = np.asarray(X, np.float64)
    return torch.from_numpy(np.ascontiguousarray(X.T).copy()).cuda().t()


def to_host(T):
    return T.cpu().numpy() if hasattr(T, "cpu") else np.asarray(T)


def strided(values, ld, lead):
    """(view, whole, check): the (n, k) `values` as a column-major CUDA view with leading dimension ld at element offset `lead` of a
    guarded buffer; the ld - n pad rows between the columns hold the canary NaN and belong to `whole` (ld * k elements)"""
    import torch
    n, k = values.shape
    flat = np.empty(ld * k)
    flat.view(np.uint64)[:] = PAD_BITS
    for r in range(k):
        flat[r * ld:r * ld + n] = values[:, r]
    g = guarded(torch.from_numpy(flat).cuda(), lead)
    return torch.as_strided(g.view, (n, k), (1, ld)), g.view, g.check


def pads_intact(whole, n, ld, k):
    w = whole.cpu().numpy().view(np.uint64).reshape(k, ld)
    return bool(np.all(w[:, n:] == PAD_BITS))


def stats(P):
    out = (C.c_int64 * 4)()
    assert P.A._d.lib.esp_precon_many_stats(P._p, out) == 0
    return tuple(int(x) for x in out)


def layered(widths, seed=3):
    """the symmetric, diagonally dominant matrix of the module's docstring, as scipy CSC"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(widths)])
    n = int(off[-1])
    edges = {}
    for l in range(1, len(widths)):
        prev, cur = widths[l - 1], widths[l]
        chosen = np.zeros(prev, bool)
        for q in range(cur):
            preds = {q % prev} | set(int(x) for x in rng.integers(0, prev, size=int(rng.integers(0, 3))))
            assert 1 <= len(preds) <= 3
            for r in preds:
                chosen[r] = True
                edges[(off[l] + q, off[l - 1] + r)] = -(0.5 + 0.5 * rng.random())
        for r in np.flatnonzero(~chosen):
            edges[(off[l] + r % cur, off[l - 1] + r)] = -(0.5 + 0.5 * rng.random())
    if edges:
        ij = np.array(list(edges), np.int64)
        v = np.array(list(edges.values()))
        S = sp.csc_matrix((np.concatenate([v, v]), (np.concatenate([ij[:, 0], ij[:, 1]]), np.concatenate([ij[:, 1], ij[:, 0]]))), shape=(n, n))
    else:
        S = sp.csc_matrix((n, n))
    return sp.csc_matrix(S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0 + rng.random(n)))


def launch_list(widths):
    """(wide, thin) launches of a schedule with these level widths: iluam.hip's rule restated"""
    wide = thin = 0
    l = 0
    while l < len(widths):
        if widths[l] > LT:
            wide += 1
            l += 1
            continue
        total = 0
        while l < len(widths) and total + widths[l] <= LT:
            total += widths[l]
            l += 1
        thin += 1
    return wide, thin


def make_matrix(esp, name):
    if name == "empty":
        return esp.ExtendableSparseMatrix(0, 0)
    if name == "fdrand987":
        return esp.fdrand(9, 8, 7)
    return from_scipy(esp, layered(WIDTHS[name]))


def rhs(n, k, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, k)))


@pytest.fixture(scope="module", params=CASES)
def case(request, esp, model):
    """(name, A, host CSC arrays, P, V with KMAX columns, the single call's columns, the model's columns): made once, never changed"""
    name = request.param
    A = make_matrix(esp, name)
    n = A.n
    arrays = host_arrays(A)
    P = esp.ILUAMPreconditioner(A)
    V = rhs(n, KMAX, 7)
    single = np.empty((n, KMAX), order="F")
    want = np.empty((n, KMAX), order="F")
    if n:
        _, diag = model.factor(arrays)
        f = P.factor()                                              # the device's own factor
        for r in range(KMAX):
            single[:, r] = P.ldiv(np.ascontiguousarray(V[:, r]))
            want[:, r] = model.ldiv(arrays, f, diag, V[:, r])
    for a in (V, single, want):
        a.setflags(write=False)
    yield name, A, arrays, P, V, single, want
    P.close()


# ---- 1. the schedules have the prescribed widths ------------------------------------------------------------------------------------------------
def schedule_widths(arrays):
    cp, rv, _ = arrays
    if len(cp) == 1:
        return [], []
    _, fwd, bwd = level_schedules(cp, rv)
    return list(np.bincount(fwd)), list(np.bincount(bwd))


def test_prescribed_level_widths(case):
    name, A, arrays, P, V, single, want = case
    fwd, bwd = schedule_widths(arrays)
    if name in WIDTHS:
        assert fwd == WIDTHS[name] and bwd == WIDTHS[name][::-1]
        assert A.n <= 2000
    assert P.levels()[1:] == (len(fwd), len(bwd))
    assert P.launches()[1] == launch_list(fwd) and P.launches()[2] == launch_list(bwd)
    expect = {"w255": (0, 1), "w256": (0, 1), "w257": (1, 0), "one_thin": (0, 1), "two_thin": (0, 2), "wide_1_wide": (2, 1),
              "chain300": (0, 2), "empty": (0, 0)}
    if name in expect:
        assert P.launches()[1] == expect[name], name
    if name == "chain300":                                          # thin launches of 256 + 44 levels
        assert fwd == [1] * 300 and P.levels()[1:] == (300, 300)


def test_the_single_call_is_the_model(case):
    name, A, arrays, P, V, single, want = case
    assert same_bits(single, want)


# ---- 2. every column, every k, every way in ------------------------------------------------------------------------------------------------------
def level_launches(P):
    la = P.launches()
    return sum(la[1]) + sum(la[2])


def check_stats(P, k, what):
    st = stats(P)
    if k == 1:
        assert st[0] == 0, (what, st)
    elif k >= 2:
        chunks = -(-k // MC)
        assert st == (2, k - (chunks - 1) * MC, level_launches(P), chunks), (what, st)


@pytest.mark.parametrize("form", FORMS)
def test_columns_bit_for_bit(case, form):
    name, A, arrays, P, V, single, want = case
    n = A.n
    for k in KS:
        what = (name, form, k)
        Vk = V[:, :k]
        if form == "host_f":
            got = P.ldiv(np.asfortranarray(Vk).copy(order="F"))
            assert isinstance(got, np.ndarray) and got.shape == (n, k)
        elif form == "host_c":
            Vc = np.ascontiguousarray(Vk).copy(order="C")
            got = P.ldiv(Vc)
            assert got.shape == (n, k) and same_bits(Vc, Vk)
        elif form == "device":
            T = to_device(Vk)
            got = P.ldiv(T)
            assert got.is_cuda and same_bits(to_host(T), Vk)        # V is not written
            got = to_host(got)
        elif form == "inplace":
            T = to_device(Vk)
            assert P.ldiv(T, out=T) is T
            got = to_host(T)
        else:
            ld = n + 3
            v, vwhole, vcheck = strided(np.asarray(Vk), ld, 1)     # an odd offset: 8 bytes off a 16-byte boundary
            u, uwhole, ucheck = strided(np.full((n, k), 7.0), ld, 3)
            assert P.ldiv(v, out=u) is u
            A.synchronize()
            got = to_host(u)
            assert same_bits(to_host(v), Vk), what
            assert pads_intact(vwhole, n, ld, k) and pads_intact(uwhole, n, ld, k), what
            vcheck("V"), ucheck("U")
        check_stats(P, k, what)
        assert not np.any(np.isnan(got)), what
        assert same_bits(got, single[:, :k]), (what, "single")
        assert same_bits(got, want[:, :k]), (what, "model")


def test_stats_refuse_null(esp, case):
    name, A, arrays, P, V, single, want = case
    lib = A._d.lib
    out = (C.c_int64 * 4)()
    assert lib.esp_precon_many_stats(None, out) == -1 and lib.esp_precon_many_stats(P._p, None) == -1


# ---- 3. the kinds that end in ILUAM -------------------------------------------------------------------------------------------------------------
def descending_interleaved(n):
    down = np.arange(n, 0, -1)
    return [down[::2], down[1::2]]


def halves(n):
    return [range(1, n // 2 + 1), range(n // 2 + 1, n + 1)]


KINDS = {
    "iluk1": lambda esp, A: esp.ILUKPreconditioner(A, 1),
    "ilut": lambda esp, A: esp.ILUTPreconditioner(A),
    "colored": lambda esp, A: esp.ColoredPreconditioner(A, esp.ILUAMPreconditioner),
    "parallel_ilu0": lambda esp, A: esp.ParallelILU0Preconditioner(A),
    "block_increasing": lambda esp, A: esp.BlockPreconditioner(A, halves(A.n), esp.ILUAMPreconditioner),
    "block_interleaved": lambda esp, A: esp.BlockPreconditioner(A, descending_interleaved(A.n), esp.ILUAMPreconditioner),
    "block_interleaved_ilu0": lambda esp, A: esp.BlockPreconditioner(A, descending_interleaved(A.n), esp.ILU0Preconditioner),
    "lu_columns": lambda esp, A: esp.LUFactorization(A, 16, form="columns"),
}
COLUMNWISE = {
    "amg": lambda esp, A: esp.AMGPreconditioner(A, max_coarse=16),
    "spai1": lambda esp, A: esp.SPAIPreconditioner(A, order=1),
}


def check_kind(esp, P, A, form, levels):
    n = A.n
    V = rhs(n, MC + 1, 5)
    single = np.empty((n, MC + 1), order="F")
    for r in range(MC + 1):
        single[:, r] = P.ldiv(np.ascontiguousarray(V[:, r]))
    for k in (2, MC, MC + 1):
        Vk = np.asfortranarray(V[:, :k])
        chunks = -(-k // MC)
        expect = (form, k - (chunks - 1) * MC, level_launches(P) if levels else 0, chunks)
        assert same_bits(P.ldiv(Vk), single[:, :k]), (k, "host")
        assert stats(P) == expect, (k, "host", stats(P))
        T = to_device(Vk)
        assert same_bits(to_host(P.ldiv(T)), single[:, :k]), (k, "device")
        assert stats(P) == expect, (k, "device", stats(P))
        assert P.ldiv(T, out=T) is T and same_bits(to_host(T), single[:, :k]), (k, "device in place")
    P.ldiv(np.asfortranarray(V[:, :1]))
    assert stats(P)[0] == 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_kinds_that_end_in_iluam(esp, kind):
    A = esp.fdrand(5, 4, 3)
    P = KINDS[kind](esp, A)
    try:
        if kind.startswith("block"):
            assert P.path == (0 if kind == "block_increasing" else 1)
        inner_ilu0 = kind in ("parallel_ilu0", "block_interleaved_ilu0")
        if not inner_ilu0:
            assert level_launches(P) > 0
        check_kind(esp, P, A, 2, not inner_ilu0)
    finally:
        P.close()


@pytest.mark.parametrize("kind", sorted(COLUMNWISE))
def test_amg_and_spai1_stay_column_by_column(esp, kind):
    A = esp.fdrand(5, 4, 3)
    P = COLUMNWISE[kind](esp, A)
    try:
        check_kind(esp, P, A, 1, False)
    finally:
        P.close()


def test_backslash(esp, monkeypatch):
    """A.solve(B) is a one-shot LUFactorization(form="columns"): its record is read just before it is closed"""
    A = esp.fdrand(6, 6, 6)
    n = A.n
    seen = []
    close = esp.LUFactorization.close

    def recording_close(self):
        if self._p is not None:
            seen.append((stats(self), level_launches(self)))
        close(self)

    monkeypatch.setattr(esp.LUFactorization, "close", recording_close)
    B = rhs(n, MC + 1, 9)
    X = A.solve(B)
    assert len(seen) == 1 and seen[0][1] > 0 and seen[0][0] == (2, 1, seen[0][1], 2), seen
    T = to_host(A.solve(to_device(B)))
    assert seen[1][0] == (2, 1, seen[1][1], 2)
    for r in range(MC + 1):
        x = A.solve(np.ascontiguousarray(B[:, r]))
        assert same_bits(X[:, r], x) and same_bits(T[:, r], x), r
    assert all(s[0][0] == 0 for s in seen[2:])


# ---- 4. cg(A, B) and gmres(A, B) ------------------------------------------------------------------------------------------------------------------
def staggered_columns(S, seed=23):
    """9 columns that stop at different iterations under reltol = 0, abstol = 1e-3 (the construction of test_cg_many_gpu.py): `zero`
    at once, `tiny` below the tolerance from the start, `axis` (A e_j scaled: one preconditioned step from its solution where the
    preconditioner is exact on it) and `small` early, the random ones later, `never` (scaled by 1e30) not within any maxiter"""
    n = S.shape[0]
    rng = np.random.default_rng(seed)
    e = np.zeros(n)
    e[n // 3] = 1.0
    return {"zero": np.zeros(n), "tiny": 1e-12 * rng.standard_normal(n), "axis": 1e-3 * (S @ e),
            "small": 1e-3 * rng.standard_normal(n), "rand1": rng.standard_normal(n), "rand2": 1e3 * rng.standard_normal(n),
            "rand3": rng.standard_normal(n), "never": 1e30 * rng.standard_normal(n), "rand4": 10.0 * rng.standard_normal(n)}


ORDER = ["rand1", "rand2", "zero", "axis", "tiny", "never", "small", "rand3", "rand4"]
CAP = 150
SOLVERS = {
    "cg": (lambda esp: esp.cg, {}, ("iters", "isconverged")),
    "gmres": (lambda esp: esp.gmres, {"restart": 5}, ("iters", "mvps", "reorth", "isconverged")),
}
KRYLOV_PRECONS = {
    "iluam": lambda esp, A: esp.ILUAMPreconditioner(A),
    "colored": lambda esp, A: esp.ColoredPreconditioner(A, esp.ILUAMPreconditioner),
}


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


def single_solves(solve, A, P, B, keys, **kw):
    out = []
    for r in range(B.shape[1]):
        x, log = solve(A, np.ascontiguousarray(B[:, r]), Pl=P, log=True, **kw)
        out.append((np.array(x), history_of(log), tuple(log[c] for c in keys)))
    return out


def assert_solves(X, logs, want, keys, what):
    assert X.shape[1] == len(logs) == len(want), what
    for r, (wx, wh, wc) in enumerate(want):
        assert tuple(logs[r][c] for c in keys) == wc, (what, r, logs[r], wc)
        assert len(logs[r]["resnorm"]) == wc[0], (what, r)
        assert same_bits(history_of(logs[r]), wh), (what, r, "history")
        assert same_bits(X[:, r], wx), (what, r, "x")


def krylov_matrix(esp, name):
    if name == "chain300":
        S = layered(WIDTHS[name])
        return from_scipy(esp, S), S
    A = esp.fdrand(9, 8, 7)
    cp, rv, nz = host_arrays(A)
    return A, sp.csc_matrix((nz, rv - 1, cp - 1), shape=(A.n, A.n))


@pytest.mark.parametrize("precon", sorted(KRYLOV_PRECONS))
@pytest.mark.parametrize("name", ["chain300", "fdrand987"])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_krylov_columns_that_stop_at_different_times(esp, solver, name, precon):
    get, extra, keys = SOLVERS[solver]
    solve = get(esp)
    A, S = krylov_matrix(esp, name)
    cols = staggered_columns(S)
    P = KRYLOV_PRECONS[precon](esp, A)
    try:
        B = np.stack([cols[c] for c in ORDER], axis=1)
        base = dict(reltol=0.0, abstol=1e-3, **extra)
        probe = dict(zip(ORDER, single_solves(solve, A, P, B, keys, maxiter=CAP, **base)))
        # `never` does stop where the preconditioner is the exact inverse (ILUAM of the chain, a tridiagonal matrix: the residual
        # reaches 0.0); everywhere else it runs to maxiter, two more than the slowest column that stops needs
        stops = [c for c in ORDER if probe[c][2][-1]]
        assert set(ORDER) - set(stops) <= {"never"}
        slowest = max(probe[c][2][0] for c in stops)
        assert slowest + 2 < CAP
        kw = dict(maxiter=slowest + 2, **base)
        single = single_solves(solve, A, P, B, keys, **kw)
        iters = dict(zip(ORDER, (s[2][0] for s in single)))
        print(solver, name, precon, iters)
        assert iters["zero"] == 0 and iters["tiny"] == 0
        if "never" not in stops:
            assert iters["never"] == kw["maxiter"] and not single[ORDER.index("never")][2][-1]
        assert len(set(iters.values())) >= 3                         # the live mask gets holes while the level launches still run
        for k in (MC, MC + 1):                                        # one chunk; a chunk and a lone column
            X, logs = solve(A, np.asfortranarray(B[:, :k]), Pl=P, log=True, **kw)
            assert_solves(X, logs, single[:k], keys, (solver, name, precon, k, "host"))
            st = stats(P)
            assert st == (2, k - (k > MC) * MC, level_launches(P), 1 + (k > MC)), st   # one column's launch count
            X, logs = solve(A, to_device(B[:, :k]), Pl=P, log=True, **kw)
            assert_solves(to_host(X), logs, single[:k], keys, (solver, name, precon, k, "torch"))
        solve(A, np.asfortranarray(B[:, :1]), Pl=P, **kw)
        assert stats(P)[0] == 0                                       # k == 1
    finally:
        P.close()


@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_a_nan_column_runs_to_maxiter_beside_the_others(esp, solver):
    get, extra, keys = SOLVERS[solver]
    solve = get(esp)
    A = esp.fdrand(9, 8, 7)
    B = rhs(A.n, MC, 6).copy(order="F")
    B[7, 2] = np.nan
    P = esp.ILUAMPreconditioner(A)
    try:
        kw = dict(maxiter=120, **extra)
        single = single_solves(solve, A, P, B, keys, **kw)
        assert single[2][2][0] == 120 and not single[2][2][-1]
        # (GMRES(5) need not bring every neighbour below the default tolerance within maxiter: one that stops early is enough for the
        # NaN column to run on beside frozen ones)
        assert any(s[2][-1] and s[2][0] < 120 for r, s in enumerate(single) if r != 2)
        X, logs = solve(A, to_device(B), Pl=P, log=True, **kw)
        X = to_host(X)
        assert_solves(X, logs, single, keys, ("nan column", solver))
        assert np.all(np.isfinite(np.delete(X, 2, axis=1)))
        assert stats(P) == (2, MC, level_launches(P), 1)
    finally:
        P.close()
