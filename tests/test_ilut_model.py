"""CPU: the normative model of ILUTPreconditioner (tests/ilut_model.c: threshold ILU by synchronous sweeps, entry by entry) is held to
account -- against a dense NumPy restatement, against iluam_model.c at the fixed point (bit for bit), on the cases where the answer
is known (tau = 0, a huge tau, the fill guard) and on what it is for (fewer Krylov iterations than ILU0) -- and the new entry
points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import block_precon_modellib
import gmres_modellib
from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel
from ilut_modellib import FillRefused, Model, dense_from, dense_ilut, restricted
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("ilut_model"))


@pytest.fixture(scope="module")
def solver_lib(tmp_path_factory):
    return block_precon_modellib.Model(tmp_path_factory.mktemp("ilut_solver_model"))


@pytest.fixture(scope="module")
def gmres_lib(tmp_path_factory):
    return gmres_modellib.Model(tmp_path_factory.mktemp("ilut_gmres_model"))


def csc_of(S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def dominant(rng, n, symmetric, density):
    """a seeded strictly diagonally dominant matrix (by rows and by columns) with a symmetric or unsymmetric pattern"""
    M = np.where(rng.random((n, n)) < density, rng.standard_normal((n, n)), 0.0)
    if symmetric:
        M = np.where(M != 0, M, M.T)                 # the pattern of M | M', other values on both sides
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    return csc_of(sp.csc_matrix(M))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# (a) ------------------------------------------------------------------------------------------------------------------------------
def test_model_equals_dense_restatement(model):
    """240 seeded diagonally dominant matrices, n <= 40, symmetric and unsymmetric patterns: the patterns are equal, the values agree
    to 1e-12 relative to the largest entry.  The restatement sums with np.dot, another order: a sum of at most 40 products differs by
    at most 40 eps times the sum of their magnitudes, which diagonal dominance keeps below the pivot; at most 12 sweeps follow each
    other, and the quotients by pivots >= 1 amplify nothing: 40 * 12 * 1.1e-16 = 5e-14, times 20 for the entries that feed later ones.
    The largest difference seen is printed (NOTES/ilut.md records it)"""
    rng = np.random.default_rng(40)
    worst = 0.0
    for trial in range(240):
        n = int(rng.integers(1, 41))
        csc = dominant(rng, n, trial % 2 == 0, rng.choice([0.05, 0.1, 0.2]))
        tau = [0.0, 1e-3, 1e-2, 0.1][trial % 4]
        steps, sweeps = [(0, 2), (1, 1), (2, 3), (3, 2)][(trial // 4) % 4]
        P = model.precon(csc, tau, steps, sweeps, max_fill=1e6)
        Pd, Fd = dense_ilut(csc, tau, steps, sweeps)
        Pm, Fm = dense_from(P.S, P.F, n)
        assert np.array_equal(Pm, Pd), (trial, n, tau, steps)
        err = np.abs(Fm - Fd).max() / np.abs(Fd).max()
        worst = max(worst, err)
        assert err <= 1e-12, (trial, n, tau, steps, err)
    print("model against the dense restatement: largest relative difference %.3e" % worst)


# (b), (c) ---------------------------------------------------------------------------------------------------------------------------
def test_fixed_point_on_the_pattern_of_a_is_iluam(model, orc):
    O = orc.fdrand(5, 4, 3, style=orc.KIND_UPDATE)
    cases = [tuple(np.array(a) for a in O.sparse().arrays())]
    rng = np.random.default_rng(41)
    cases += [dominant(rng, 25, s, 0.15) for s in (True, False)]
    for csc in cases:
        n = len(csc[0]) - 1
        P = model.precon(csc, 0.5, 0, 2 * n)
        want, _ = model.iluam.factor(csc)
        assert np.array_equal(P.S[0], csc[0]) and np.array_equal(P.S[1], csc[1]) and same_bits(P.F, want)
        assert same_bits(P.sweep(1).F, want)                       # ... and it is a fixed point


@pytest.mark.parametrize("tau", [0.0, 1e-3, 1e-2, 0.3])
@pytest.mark.parametrize("steps", [1, 3])
def test_fixed_point_on_s_is_iluam_of_a_restricted_to_s(model, orc, tau, steps):
    O = orc.fdrand(5, 4, 3, style=orc.KIND_UPDATE)
    cases = [tuple(np.array(a) for a in O.sparse().arrays()), dominant(np.random.default_rng(42), 30, False, 0.12)]
    for csc in cases:
        n = len(csc[0]) - 1
        P = model.precon(csc, tau, steps, 2, max_fill=1e6)
        P.sweep(2 * n)
        want, _ = model.iluam.factor(restricted(csc, P.S))
        assert same_bits(P.F, want)


# (d) ------------------------------------------------------------------------------------------------------------------------------
def test_tau_zero_drops_nothing_and_a_huge_tau_leaves_the_diagonal(model):
    csc = dominant(np.random.default_rng(43), 30, False, 0.12)
    n = 30
    P = model.precon(csc, 0.0, 2, 2, max_fill=1e6)
    assert all(c == s for c, s in P.stats) and P.stats[1][0] >= P.stats[0][0] > len(csc[1])
    P = model.precon(csc, 1e300, 2, 2)
    assert np.array_equal(P.S[0], np.arange(1, n + 2)) and np.array_equal(P.S[1], np.arange(1, n + 1))
    A = sp.csc_matrix((csc[2], csc[1] - 1, csc[0] - 1), shape=(n, n))
    assert same_bits(P.F, A.diagonal())                            # u_jj = a_jj: nothing is left to subtract
    nan = tuple(a.copy() for a in csc)
    q = int(np.flatnonzero(csc[1] != np.repeat(np.arange(1, n + 1), np.diff(csc[0])))[3])
    nan[2][q] = np.nan                                             # fabs(NaN) < tau is false: a NaN is kept
    P = model.precon(nan, 1e300, 1, 1, max_fill=1e6)
    assert np.isnan(P.F).any() and len(P.S[1]) > n


# (e) ------------------------------------------------------------------------------------------------------------------------------
class SolverModel(BlockModel):
    """BlockModel's statement-by-statement solvers driven with any ldiv and A's mul"""

    def __init__(self, lib, csc, ldiv):
        self.m, self.csc, self.n, self._ldiv = lib, tuple(np.array(a, copy=True) for a in csc), len(csc[0]) - 1, ldiv

    def ldiv(self, v):
        return self._ldiv(np.ascontiguousarray(v, np.float64))


def ilu0_model(lib, csc, orc):
    P = lib.precon("ilu0", csc, orc)
    return SolverModel(lib, csc, lambda v: lib.ldiv(P, csc, v))


def test_cg_needs_fewer_iterations_than_ilu0(model, solver_lib, orc):
    """fdrand 8^3, b = A*ones, reltol 1e-8"""
    O = orc.fdrand(8, 8, 8, style=orc.KIND_UPDATE)
    csc = tuple(np.array(a) for a in O.sparse().arrays())
    b = solver_lib.mul(csc, np.ones(512))
    P = model.precon(csc, 1e-2, 3, 3)
    _, _, it_t, conv_t = SolverModel(solver_lib, csc, P.ldiv).cg(b, reltol=1e-8)
    _, _, it_0, conv_0 = ilu0_model(solver_lib, csc, orc).cg(b, reltol=1e-8)
    print("cg on fdrand 8^3: ILU0 %d iterations, ILUT(1e-2, 3, 3) %d, nnz(F)/nnz(A) = %.2f" % (it_0, it_t, len(P.S[1]) / len(csc[1])))
    assert conv_t and conv_0 and it_t < it_0


def test_gmres_needs_fewer_iterations_than_ilu0(model, solver_lib, gmres_lib, orc):
    """convdiff(8, 8, 8) at Pe 4, b = A*ones, reltol 1e-8, gmres(20)"""
    I, J, V = convdiff_triplets(8, 8, 8, 4.0)
    csc = csc_of(sp.csc_matrix((V, (I - 1, J - 1)), shape=(512, 512)))
    b = solver_lib.mul(csc, np.ones(512))
    P = model.precon(csc, 1e-2, 3, 3)
    t = gmres_lib.gmres_cb(SolverModel(solver_lib, csc, P.ldiv), 512, b, restart=20, reltol=1e-8)
    z = gmres_lib.gmres_cb(ilu0_model(solver_lib, csc, orc), 512, b, restart=20, reltol=1e-8)
    print("gmres(20) on convdiff 8^3, Pe 4: ILU0 %d iterations, ILUT(1e-2, 3, 3) %d, nnz(F)/nnz(A) = %.2f"
          % (z.iters, t.iters, len(P.S[1]) / len(csc[1])))
    assert t.converged and z.converged and t.iters < z.iters


# (f) ------------------------------------------------------------------------------------------------------------------------------
def test_fill_guard_fires_at_the_stated_count(model):
    csc = dominant(np.random.default_rng(44), 30, False, 0.12)
    nnz = len(csc[1])
    P = model.precon(csc, 1e-3, 2, 1, max_fill=1e6)
    c0 = P.stats[0][0]
    assert c0 > nnz
    model.precon(csc, 1e-3, 1, 1, max_fill=(c0 + 0.5) / nnz)                  # the limit is nnz(C): accepted
    with pytest.raises(FillRefused) as e:
        model.precon(csc, 1e-3, 1, 1, max_fill=(c0 - 0.5) / nnz)              # one below: refused
    assert (e.value.step, e.value.nnz_c, e.value.limit) == (0, c0, c0 - 1)
    c1 = P.stats[1][0]
    if c1 > c0:
        with pytest.raises(FillRefused) as e:
            model.precon(csc, 1e-3, 2, 1, max_fill=(c1 - 0.5) / nnz)
        assert (e.value.step, e.value.nnz_c) == (1, c1)


def test_warm_update_carries_the_state(model):
    """keep_pattern: the pattern stays, F starts from its current values; without it the construction runs again"""
    csc = dominant(np.random.default_rng(45), 30, False, 0.12)
    new = (csc[0], csc[1], csc[2] * (1.0 + 0.01 * np.random.default_rng(46).random(len(csc[2]))))
    W, F = model.precon(csc, 1e-2, 2, 2, keep_pattern=True), model.precon(csc, 1e-2, 2, 2)
    S, F0 = W.S, W.F.copy()
    W.update(new)
    F.update(new)
    assert W.S is S and not same_bits(W.F, F0) and W.sweeps_run == 2
    fresh = model.precon(new, 1e-2, 2, 2)
    assert np.array_equal(F.S[1], fresh.S[1]) and same_bits(F.F, fresh.F)
    W.update(new)                                                    # a second warm update moves on from the first
    assert W.S is S


def test_a_missing_diagonal_is_refused(model):
    csc = csc_of(sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))
    with pytest.raises(ValueError):
        model.precon(csc)


def test_ilut_entry_points_declared_and_exported(esp):
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_ILUT\s+8\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = esp._lib.load()
    for name in ("esp_precon_ilut_create", "esp_precon_ilut_matrix", "esp_precon_ilut_stats", "esp_precon_ilut_limits"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    for name in ("ESP_ILUT_WAVE_UPPER", "ESP_ILUT_GROUP_UPPER", "ESP_ILUT_STEPS_MAX", "ESP_ILUT_STATS"):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
        assert m and int(m.group(1)) == getattr(esp._lib, name)
    out = (esp._lib.i64 * 4)()
    assert lib.esp_precon_ilut_limits(out) == 0                      # (no device needed)
    assert list(out) == [esp._lib.ESP_ILUT_WAVE_UPPER, esp._lib.ESP_ILUT_GROUP_UPPER, esp._lib.ESP_ILUT_STEPS_MAX, esp._lib.ESP_ILUT_STATS]
    assert esp.ESP_PRECON_ILUT == 8 and esp.ILUTPreconditioner.KIND == 8
    with pytest.raises(TypeError):
        esp.ILUTPreconditioner("not a matrix")
    with pytest.raises(NotImplementedError):
        esp.AMGCL_RLXPreconditioner("not a matrix", type="ilut")
