"""GPU: the solve side at the edges of its compile-time capacities, on the crafted patterns of tests/edge_patterns.py.
1. ILUAM's launch list (iluam.hip, LT = 256): levels of 256 / 257 nodes, folds of exactly 256 / 257 nodes, thin groups between wide
   launches -- launches() against the rule restated in Python, factor(), ldiv!, simple! and a values-only update! bitwise the model of
   tests/iluam_model.c; ILU(0) by ILUKPreconditioner and BlockPreconditioner over ILUAM on the same pattern.
2. The staged row kernels (precon.hip PCAP, krylov.hpp KCAP = 2048): 256-row blocks of 2047 / 2048 / 2049 entries in A's row-wise
   index and in ILU0's two parts, a single row above the capacity, an empty part, a ragged last block above it -- mul!, ILU0's ldiv!,
   simple!, cg, bicgstabl and gmres bitwise their models.
3. The solvers' grid cap (KGRID = 2048 workgroups of 256-element chunks): n = 524 545 (2050 chunks: every vector kernel takes a second
   round) and n = 1 049 089 (4099 chunks: mgs_step_k, two chunks per round, takes one too) -- cg, bicgstabl and gmres bitwise their
   models; n = 65 537 (257 partials in norm_finish_k) for simple!.
Every comparison is on bits; simple!'s residual norms are held to the rtol of test_precon_gpu.py's test_simple_bitwise (1e-13)."""
import numpy as np
import pytest

import block_precon_modellib
import edge_patterns as ep
import gmres_modellib
import iluk_modellib
import precon_modellib
from block_precon_modellib import BlockModel
from iluam_modellib import level_schedules
from refmodel import bits

pytestmark = pytest.mark.gpu

KINDS = ["identity", "jacobi", "ilu0"]
ORTHS = ["mgs", "cgs", "dgks"]
SIMPLE_RTOL = 1e-13      # test_precon_gpu.py::test_simple_bitwise, test_iluam_gpu.py::test_simple_bitwise: the same residual kernel
N1 = 2048 * 256 + 257    # 2050 chunks, the last of one row
N2 = 4098 * 256 + 1      # 4099 chunks: 2050 spans of mgs_step_k, the last of one chunk of one element
N3 = 65537               # 257 partials in norm_finish_k


# ---- the models, each compiled once --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ik(tmp_path_factory):
    """iluk_model.c; .iluam is iluam_model.c's Model"""
    return iluk_modellib.Model(tmp_path_factory.mktemp("edges_iluk_model"))


@pytest.fixture(scope="module")
def sm(tmp_path_factory):
    """cg_model.c and bicgstabl_model.c: precon, ldiv, mul, dot, cg, bicgstabl"""
    return block_precon_modellib.Model(tmp_path_factory.mktemp("edges_solver_model"))


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("edges_gmres_model"))


@pytest.fixture(scope="module")
def pm(tmp_path_factory):
    return precon_modellib.Model(tmp_path_factory.mktemp("edges_precon_model"))


def host_arrays(A):
    """copies of the CSC arrays (the host copy behind A.sparse() is refreshed in place by later reads)"""
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def finite_and_same(got, want):
    """the crafted patterns are diagonally dominant: nothing is non-finite, so the bits decide alone"""
    want = np.asarray(want, np.float64)
    return bool(np.isfinite(want).all()) and same_bits(got, want)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64).copy()).cuda()


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


def make_precon(esp, A, kind):
    return {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner}[kind](A)


def close(P):
    if P is not None:
        P.close()


def rule(cp, rv):
    """(levels, launches) of the three schedules of a pattern: level_schedules and the launch rule applied to its widths"""
    sched = level_schedules(cp, rv)
    return tuple(int(l.max()) + 1 for l in sched), tuple(ep.launch_list(ep.widths_of(l)) for l in sched)


# =================================================================================================================================
# 1. level launches
# =================================================================================================================================
LAYERED = {}     # (name, form) -> (A, arrays, P, factor, diag, levels, launches): built once, never changed


def layered_case(esp, ik, name, form):
    key = (name, form)
    if key not in LAYERED:
        I, J, V, n = ep.layered(ep.WIDTHS[name], form, seed=3)
        A = ep.from_triplets(esp, n, I, J, V)
        arrays = host_arrays(A)
        want = ep.csc_arrays(n, I, J, V)
        assert np.array_equal(arrays[0], want[0]) and np.array_equal(arrays[1], want[1]) and same_bits(arrays[2], want[2])
        f, diag = ik.iluam.factor(arrays)
        LAYERED[key] = (A, arrays, esp.ILUAMPreconditioner(A), f, diag) + rule(arrays[0], arrays[1])
    return LAYERED[key]


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    yield
    for case in LAYERED.values():
        case[2].close()
    LAYERED.clear()
    STAGED.clear()
    GRID.clear()


layered_params = pytest.mark.parametrize("name,form", [(name, form) for name in ep.WIDTHS for form in ep.FORMS])


@layered_params
def test_levels_and_launches(esp, ik, name, form):
    """levels() and launches() against level_schedules and the launch rule; the prescribed schedule has the prescribed widths"""
    A, arrays, P, f, diag, levels, launches = layered_case(esp, ik, name, form)
    sched = level_schedules(arrays[0], arrays[1])
    for k in ep.PRESCRIBED[form]:
        assert ep.widths_of(sched[k]) == ep.WIDTHS[name]
        assert launches[k] == ep.launch_list(ep.WIDTHS[name])
    print(name, form, "levels", P.levels(), "launches", P.launches())
    assert P.levels() == levels
    assert P.launches() == launches


@layered_params
def test_layered_factor_bitwise(esp, ik, name, form):
    A, arrays, P, f, diag, levels, launches = layered_case(esp, ik, name, form)
    assert finite_and_same(P.factor(), f)


@pytest.mark.parametrize("where", ["host", "torch_aliased"])
@layered_params
def test_layered_ldiv_bitwise(esp, ik, name, form, where):
    """ldiv! of a seeded normal vector: a host vector, and a device vector aliased in place"""
    A, arrays, P, f, diag, levels, launches = layered_case(esp, ik, name, form)
    v = np.random.default_rng(1).standard_normal(A.n)
    want = ik.iluam.ldiv(arrays, f, diag, v)
    if where == "host":
        vv = v.copy()
        got = np.asarray(P.ldiv(vv))
        assert np.array_equal(vv, v)
    else:
        tv = cuda(v)
        out = P.ldiv(tv, out=tv)
        assert out.data_ptr() == tv.data_ptr()
        got = tv.cpu().numpy()
    assert finite_and_same(got, want)


@pytest.mark.parametrize("name", ["mixed", "chain300"])
def test_layered_simple_bitwise(esp, ik, name):
    """5 simple! steps with reltol = abstol = 0: u bitwise the model's, the norms to rounding"""
    A, arrays, P, f, diag, levels, launches = layered_case(esp, ik, name, "symmetric")
    rng = np.random.default_rng(6)
    b, u0 = rng.standard_normal(A.n), rng.standard_normal(A.n)
    tu = cuda(u0)
    got, log = esp.simple(A, cuda(b), u=tu, Pl=P, maxiter=5, reltol=0.0, abstol=0.0, log=True)
    wu, wh, wit = ik.iluam.simple(arrays, f, diag, b, u=u0, maxiter=5, abstol=0.0, reltol=0.0)
    assert wit == 5 and len(log["resnorm"]) == 6
    assert finite_and_same(got.cpu().numpy(), wu)
    np.testing.assert_allclose(log["resnorm"], wh, rtol=SIMPLE_RTOL, atol=0)


@pytest.mark.parametrize("name", ["mixed", "chain300"])
def test_layered_values_only_update(esp, ik, name):
    """a re-assembly that hits stored positions only, then update!: bitwise a fresh model factorization on the kept launch list"""
    I, J, V, n = ep.layered(ep.WIDTHS[name], "symmetric", seed=3)
    A = ep.from_triplets(esp, n, I, J, V)            # (a matrix of its own: the shared case stays unchanged)
    cp, rv, nz0 = host_arrays(A)
    P = esp.ILUAMPreconditioner(A)
    levels, launches = rule(cp, rv)
    assert P.levels() == levels and P.launches() == launches
    rng = np.random.default_rng(4)
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    off = np.flatnonzero(rv != cols)
    sel = rng.choice(off, len(off) // 2, replace=False)
    d = np.arange(1, n + 1)
    A.append(esp.ESP_UPDATE, np.concatenate([rv[sel], d]), np.concatenate([cols[sel], d]),
             np.concatenate([rng.uniform(-0.1, 0.1, len(sel)), np.full(n, 0.25)]))
    A.flush()
    cp1, rv1, nz1 = host_arrays(A)
    assert np.array_equal(cp1, cp) and np.array_equal(rv1, rv) and not np.array_equal(nz1, nz0)
    f0, _ = ik.iluam.factor((cp, rv, nz0))
    assert finite_and_same(P.factor(), f0)                       # no update!: the old factorization
    P.update()
    f1, diag = ik.iluam.factor((cp, rv, nz1))
    assert finite_and_same(P.factor(), f1) and not same_bits(f1, f0)
    assert P.levels() == levels and P.launches() == launches
    v = rng.standard_normal(n)
    assert finite_and_same(P.ldiv(v), ik.iluam.ldiv((cp, rv, nz1), f1, diag, v))
    P.close()


def test_mixed_iluk0(esp, ik):
    """ILUKPreconditioner(A, k=0) on mixed/symmetric: B = A, the inner ILUAM on the same launch list"""
    A, arrays, _, f, diag, levels, launches = layered_case(esp, ik, "mixed", "symmetric")
    want = ik.precon(arrays, 0)
    P = esp.ILUKPreconditioner(A, k=0)
    try:
        bcp, brv, bnz = P.fill_matrix()
        assert np.array_equal(bcp, want.B[0]) and np.array_equal(brv, want.B[1]) and same_bits(bnz, want.B[2])
        assert (P.levels(), P.launches()) == rule(bcp, brv) == (levels, launches)
        assert finite_and_same(P.factor(), want.fval)
        v = np.random.default_rng(1).standard_normal(A.n)
        u = want.ldiv(v)
        assert finite_and_same(P.ldiv(v), u)
        t = cuda(v)
        assert P.ldiv(t, out=t).data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    finally:
        P.close()


def interleaved(n):
    """two partitions, the first not increasing (1, 5, 9, .., 3, 7, 11, ..): the permuted path (test_gmres_gpu.py's)"""
    return [np.concatenate([np.arange(1, n, 4), np.arange(3, n, 4)]), np.arange(0, n, 2)]


@pytest.mark.parametrize("which", ["one_partition", "interleaved"])
def test_mixed_block_over_iluam(esp, orc, ik, sm, which):
    """BlockPreconditioner with ILUAM inside on mixed/symmetric: the identity path (one partition 1:n) and the permuted path"""
    A, arrays, _, f, diag, levels, launches = layered_case(esp, ik, "mixed", "symmetric")
    n = A.n
    parts = [np.arange(n)] if which == "one_partition" else interleaved(n)
    permuted = which == "interleaved"
    P = esp.BlockPreconditioner(A, [p + 1 for p in parts], esp.ILUAMPreconditioner)
    try:
        assert P.path == (1 if permuted else 0)
        BM = BlockModel(sm, orc, "iluam", arrays, parts)
        bcp, brv, bnz = P.block_matrix()
        wcp, wrv, wnz, _ = block_precon_modellib.block_matrix(arrays, parts, permuted)
        assert np.array_equal(bcp, wcp) and np.array_equal(brv, wrv) and same_bits(bnz, wnz)
        inner = rule(bcp, brv)
        print(which, "levels", P.levels(), "launches", P.launches())
        assert (P.levels(), P.launches()) == inner
        if not permuted:
            assert inner == (levels, launches)
        assert finite_and_same(P.factor(), BM.factor(permuted))
        v = np.random.default_rng(1).standard_normal(n)
        u = BM.ldiv(v)
        assert finite_and_same(P.ldiv(v), u)
        t = cuda(v)
        assert P.ldiv(t, out=t).data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), u)
    finally:
        P.close()


def test_mixed_colored_reports_the_inner_launches(esp, ik):
    """ColoredPreconditioner over ILUAM on mixed/symmetric: levels() and launches() are the inner preconditioner's, the rule
    applied to the schedules of A[c,c]; ldiv! bitwise the model's on A[c,c] behind the gather and the scatter"""
    A, arrays, _, f, diag, levels, launches = layered_case(esp, ik, "mixed", "symmetric")
    P = esp.ColoredPreconditioner(A)
    try:
        B = P.reordered_matrix()
        inner = rule(B[0], B[1])
        print("colored: %d colours, levels %s, launches %s" % (P.ncolors, P.levels(), P.launches()))
        assert (P.levels(), P.launches()) == inner and max(inner[0]) <= P.ncolors
        fB, dB = ik.iluam.factor(B)
        assert finite_and_same(P.factor(), fB)
        c = P.permutation() - 1
        v = np.random.default_rng(1).standard_normal(A.n)
        want = np.empty(A.n)
        want[c] = ik.iluam.ldiv(B, fB, dB, np.ascontiguousarray(v[c]))
        assert finite_and_same(P.ldiv(v), want)
    finally:
        P.close()


def test_launches_of_the_other_kinds(esp, ik):
    """zeros for the kinds that hold no ILUAM; the errors of esp_precon_levels"""
    import ctypes
    A = layered_case(esp, ik, "fold_exact", "symmetric")[0]
    lib = A._d.lib
    for cls in (esp.JacobiPreconditioner, esp.ILU0Preconditioner):
        P = cls(A)
        out = (ctypes.c_int64 * 6)(*([7] * 6))
        assert lib.esp_precon_launches(P._p, out) == 0 and list(out) == [0] * 6
        assert lib.esp_precon_launches(P._p, None) == -1
        P.close()
    out = (ctypes.c_int64 * 6)()
    assert lib.esp_precon_launches(None, out) == -1


# =================================================================================================================================
# 2. row staging
# =================================================================================================================================
STAGED = {}


def staged_case(esp):
    """the capacity matrix: (A, arrays), built once, never changed"""
    if not STAGED:
        I, J, V, n = ep.capacity(seed=7)
        A = ep.from_triplets(esp, n, I, J, V)
        arrays = host_arrays(A)
        want = ep.csc_arrays(n, I, J, V)
        assert np.array_equal(arrays[0], want[0]) and np.array_equal(arrays[1], want[1]) and same_bits(arrays[2], want[2])
        STAGED["case"] = (A, arrays)
    return STAGED["case"]


@pytest.mark.parametrize("where", ["host", "torch"])
def test_staged_mul(esp, sm, where):
    A, arrays = staged_case(esp)
    x = np.random.default_rng(3).standard_normal(A.n)
    want = sm.mul(arrays, x)
    got = np.asarray(A.mul(x)) if where == "host" else A.mul(cuda(x)).cpu().numpy()
    assert finite_and_same(got, want)


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("alias", [False, True])
def test_staged_ilu0_ldiv(esp, orc, pm, where, alias):
    A, arrays = staged_case(esp)
    cp, rv, nz = arrays
    n = A.n
    xd, idg = orc.CSC(n, n, cp, rv, nz).ilu0()
    v = np.random.default_rng(1).standard_normal(n)
    want = pm.ilu0_ldiv(arrays, xd, idg, v)
    P = esp.ILU0Preconditioner(A)
    if where == "host":
        vv = v.copy()
        got = P.ldiv(vv, out=vv if alias else None)
        assert (got is vv) if alias else np.array_equal(vv, v)
        got = np.asarray(got)
    else:
        tv = cuda(v)
        got = P.ldiv(tv, out=tv if alias else None)
        assert (got.data_ptr() == tv.data_ptr()) if alias else np.array_equal(tv.cpu().numpy(), v)
        got = got.cpu().numpy()
    assert finite_and_same(got, want)
    P.close()


def simple_against_model(esp, orc, pm, A, arrays, kind, seed):
    cp, rv, nz = arrays
    n = A.n
    Cm = orc.CSC(n, n, cp, rv, nz)
    diag, idg = (Cm.jacobi(), None) if kind == "jacobi" else Cm.ilu0()
    rng = np.random.default_rng(seed)
    b, u0 = rng.standard_normal(n), rng.standard_normal(n)
    P = make_precon(esp, A, kind)
    tu = cuda(u0)
    got, log = esp.simple(A, cuda(b), u=tu, Pl=P, maxiter=5, reltol=0.0, abstol=0.0, log=True)
    wu, wh, wit = pm.simple({"jacobi": precon_modellib.KIND_JACOBI, "ilu0": precon_modellib.KIND_ILU0}[kind], arrays, diag, idg, b,
                            u=u0, maxiter=5, abstol=0.0, reltol=0.0)
    assert wit == 5 and len(log["resnorm"]) == 6
    assert finite_and_same(got.cpu().numpy(), wu)
    np.testing.assert_allclose(log["resnorm"], wh, rtol=SIMPLE_RTOL, atol=0)
    P.close()


def test_staged_simple(esp, orc, pm):
    A, arrays = staged_case(esp)
    simple_against_model(esp, orc, pm, A, arrays, "ilu0", 6)


def solver_b(n):
    return np.random.default_rng(9).standard_normal(n)


def check_cg(esp, orc, sm, A, arrays, MP, kind, b, **kw):
    """x, the history, the iteration count and the flag bit for bit the model's"""
    P = make_precon(esp, A, kind)
    try:
        got, log = esp.cg(A, cuda(b), Pl=P, log=True, **kw)
        wx, wh, wit, wconv = sm.cg(MP, arrays, b, **kw)
        print("cg %s: %d iterations (model %d), last norm %.3e" % (kind, log["iters"], wit, history_of(log)[-1]))
        assert log["iters"] == wit and log["isconverged"] == wconv and len(log["resnorm"]) == wit
        assert finite_and_same(history_of(log), wh)
        assert finite_and_same(got.cpu().numpy(), wx)
        return log
    finally:
        close(P)


def check_bicgstabl(esp, orc, sm, A, arrays, MP, kind, b, **kw):
    P = make_precon(esp, A, kind)
    try:
        got, log = esp.bicgstabl(A, cuda(b), Pl=P, log=True, **kw)
        wx, wh, wit, wmv, wconv = sm.bicgstabl(MP, arrays, b, **kw)
        print("bicgstabl %s l=%d: %d outer iterations (model %d), %d products, last norm %.3e"
              % (kind, kw["l"], log["iters"], wit, log["mvps"], history_of(log)[-1]))
        assert log["iters"] == wit and log["mvps"] == wmv and log["isconverged"] == wconv and len(log["resnorm"]) == wit
        assert finite_and_same(history_of(log), wh)
        assert finite_and_same(got.cpu().numpy(), wx)
        return log
    finally:
        close(P)


def check_gmres(esp, orc, gm, A, arrays, MP, kind, b, **kw):
    P = make_precon(esp, A, kind)
    try:
        got, log = esp.gmres(A, cuda(b), Pl=P, log=True, **kw)
        want = gm.gmres(MP, arrays, b, **kw)
        print("gmres %s %s: %d iterations (model %d), %d products, %d correction passes (model %d), last norm %.3e"
              % (kind, kw["orth_meth"], log["iters"], want.iters, log["mvps"], log["reorth"], want.reorth, history_of(log)[-1]))
        assert log["iters"] == want.iters and log["mvps"] == want.mvps and log["reorth"] == want.reorth
        assert log["isconverged"] == want.converged and len(log["resnorm"]) == want.iters
        assert finite_and_same(history_of(log), want.history)
        assert finite_and_same(got.cpu().numpy(), want.x)
        return log
    finally:
        close(P)


@pytest.mark.parametrize("kind", KINDS)
def test_staged_cg(esp, orc, sm, kind):
    """the matrix is not symmetric: the model defines cg's arithmetic on any matrix (test_cg_gpu.py::test_nonsymmetric_pattern)"""
    A, arrays = staged_case(esp)
    log = check_cg(esp, orc, sm, A, arrays, sm.precon(kind, arrays, orc), kind, solver_b(A.n), maxiter=6, reltol=0.0)
    assert log["iters"] == 6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("l", [2, 4])
def test_staged_bicgstabl(esp, orc, sm, kind, l):
    A, arrays = staged_case(esp)
    log = check_bicgstabl(esp, orc, sm, A, arrays, sm.precon(kind, arrays, orc), kind, solver_b(A.n), l=l, max_mv_products=12, reltol=0.0)
    assert log["mvps"] >= 12


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("orth", ORTHS)
def test_staged_gmres(esp, orc, gm, kind, orth):
    A, arrays = staged_case(esp)
    log = check_gmres(esp, orc, gm, A, arrays, gm.precon(kind, arrays, orc), kind, solver_b(A.n), restart=5, maxiter=7, orth_meth=orth,
                      reltol=0.0)
    assert log["iters"] == 7


# =================================================================================================================================
# 3. grid cap
# =================================================================================================================================
GRID = {}


def grid_case(esp, orc, sm, n):
    """the tridiagonal matrix of n rows: (A, arrays, b, {kind: the model's preconditioner}), built once, never changed"""
    if n not in GRID:
        A = ep.tridiagonal(esp, n)
        arrays = host_arrays(A)
        assert A.nnz() == 3 * n - 2
        GRID[n] = (A, arrays, np.random.default_rng(n).standard_normal(n), {kind: sm.precon(kind, arrays, orc) for kind in KINDS})
    return GRID[n]


def test_grid_sizes():
    """what the sizes are chosen for: KGRID = 2048 workgroups of 256-element chunks, mgs_step_k two chunks per round"""
    for n, chunks in ((N1, 2050), (N2, 4099)):
        assert -(-n // 256) == chunks and n % 256 == 1 and n % 2 == 1
    assert -(-N1 // 256) > 2048 >= (-(-N1 // 256) + 1) // 2        # the vector kernels take a second round, mgs_step_k not yet
    assert (-(-N2 // 256) + 1) // 2 == 2050 > 2048                 # mgs_step_k too
    assert -(-N3 // 256) == 257


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [N1, N2])
def test_grid_cg(esp, orc, sm, n, kind):
    A, arrays, b, MPs = grid_case(esp, orc, sm, n)
    log = check_cg(esp, orc, sm, A, arrays, MPs[kind], kind, b, maxiter=3, reltol=0.0)
    assert log["iters"] == 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("l", [2, 4])
@pytest.mark.parametrize("n", [N1, N2])
def test_grid_bicgstabl(esp, orc, sm, n, l, kind):
    A, arrays, b, MPs = grid_case(esp, orc, sm, n)
    log = check_bicgstabl(esp, orc, sm, A, arrays, MPs[kind], kind, b, l=l, max_mv_products=8, reltol=0.0)
    assert log["mvps"] >= 8


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("n", [N1, N2])
def test_grid_gmres(esp, orc, sm, gm, n, orth, kind):
    A, arrays, b, MPs = grid_case(esp, orc, sm, n)
    log = check_gmres(esp, orc, gm, A, arrays, MPs[kind], kind, b, restart=5, maxiter=7, orth_meth=orth, reltol=0.0)
    assert log["iters"] == 7
    if orth == "dgks":
        assert log["reorth"] > 0         # the predicate kernels really ran past the cap
    else:
        assert log["reorth"] == 0


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
def test_norm_finish_257_partials(esp, orc, pm, kind):
    """n = 65 537: norm_finish_k's strided loop meets a 257th partial"""
    A = ep.tridiagonal(esp, N3)
    simple_against_model(esp, orc, pm, A, host_arrays(A), kind, 5)
