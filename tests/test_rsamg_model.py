"""CPU: the model of RS_AMGPreconditioner (tests/rsamg_model.c through tests/rsamg_modellib.py) is held to account by a second,
independent NumPy / SciPy restatement of the whole setup and cycle -- the splitting, cnum and the rounds equal, P and ldiv to 1e-12
relative -- by the invariant of the splitting on every graph, and by the two branches of the interpolation's positive part on the
posmix graph; and the new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import amg_modellib as am
import rsamg_modellib as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return rs.Model(tmp_path_factory.mktemp("rsamg_model"))


@pytest.fixture(scope="module")
def graphs(orc):
    def fd(*dims):
        O = orc.fdrand(*dims, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
        return tuple(np.array(a) for a in O.sparse().arrays())
    g = rs.graphs(fd)
    assert set(name for name, _ in rs.GRAPH_CASES) == set(g)
    return g


def scipy_of(csc):
    cp, rv, nz = csc
    n = len(cp) - 1
    return sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))


# ---- the independent restatement: whole-array NumPy / SciPy, no loop over entries, ranks instead of 64-bit keys ------------------
def mix32(i):
    x = (i.astype(np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def scipy_level(S, theta):
    """-> (cf, nc, rounds, P as a dense n x nc array) of one level"""
    n = S.shape[0]
    A = np.asarray(S.todense(), dtype=np.float64)
    off = A.copy()
    np.fill_diagonal(off, 0.0)
    with np.errstate(invalid="ignore"):
        absoff = np.abs(off)
        m = np.where(np.isnan(absoff), 0.0, absoff).max(axis=1) if n else np.zeros(0)
        dep = (absoff != 0) & (absoff >= theta * m[:, None])          # dep[i, j]: i depends on j (a NaN compares false)
    lam = dep.sum(axis=0)
    idx = np.arange(n)
    # the order of the keys: lambda capped, then the upper 16 bits of the mixer, then the index
    order = np.lexsort((idx, mix32(idx) >> np.uint64(16), np.minimum(lam, 65535)))
    rank = np.empty(n, np.int64)
    rank[order] = idx + 1
    nbr = dep | dep.T
    state = np.where(dep.any(axis=1), 0, 3)
    rounds = 0
    while (state == 0).any():
        und = state == 0
        best = (nbr * np.where(und, rank, 0)[None, :]).max(axis=1)
        newc = und & (rank > best)
        isc = (state == 1) | newc
        hasc = (dep & isc[None, :]).any(axis=1)
        state = np.where(newc, 1, np.where(und & hasc, 2, state))
        rounds += 1
    isc = state == 1
    cnum = np.cumsum(isc) - 1
    nc = int(isc.sum())
    cf = np.where(isc, cnum, np.where(state == 2, -1, -2))
    # direct interpolation
    with np.errstate(all="ignore"):
        neg, pos = np.minimum(off, 0.0), np.maximum(off, 0.0)
        neg, pos = np.where(np.isnan(neg), 0.0, neg), np.where(np.isnan(pos), 0.0, pos)
        inc = dep & isc[None, :]
        sn, sp_ = neg.sum(axis=1), pos.sum(axis=1)
        snc, spc = (neg * inc).sum(axis=1), (pos * inc).sum(axis=1)
        d = np.diag(A).copy()
        d = np.where(spc == 0, d + sp_, d)
        beta = np.where(spc == 0, 0.0, sp_ / np.where(spc == 0, 1.0, spc))
        alpha = np.where(snc != 0, sn / np.where(snc != 0, snc, 1.0), 0.0)
        W = -(alpha[:, None] * (neg * inc) + beta[:, None] * (pos * inc)) / d[:, None]
    P = np.zeros((n, nc))
    f = state == 2
    P[f] = W[f][:, isc]
    P[idx[isc], cnum[isc]] = 1.0
    return cf, nc, rounds, P


class ScipyRS:
    def __init__(self, S, theta=0.25, max_levels=10, max_coarse=64, presweeps=1, postsweeps=1):
        self.pre, self.post = presweeps, postsweeps
        self.levels, self.inv = [], None
        A = np.asarray(sp.csc_matrix(S).todense(), dtype=np.float64)
        while True:
            n = A.shape[0]
            with np.errstate(all="ignore"):
                d = np.diag(A)
                rho = np.float64(np.abs(A / d[:, None]).sum(axis=1).max() if n else 0.0)
                L = {"A": A, "w": (np.float64(4.0 / 3.0) / rho) / d, "cf": None, "P": None, "rounds": 0}
            self.levels.append(L)
            coarsest = n <= max_coarse or len(self.levels) == max_levels
            if not coarsest:
                L["cf"], nc, L["rounds"], P = scipy_level(sp.csc_matrix(A), theta)
                coarsest = nc == 0 or nc == n
            if coarsest:
                if n <= am.DENSE_MAX:
                    self.inv = np.linalg.inv(A) if n else np.zeros((0, 0))
                break
            L["P"] = P
            A = P.T @ A @ P

    def cycle(self, l, b):
        L = self.levels[l]
        last = l + 1 == len(self.levels)
        if last and self.inv is not None:
            return self.inv @ b
        A, w = L["A"], L["w"]
        x = w * b
        for _ in range(1, self.pre):
            x = x + w * (b - A @ x)
        if not last:
            x = x + L["P"] @ self.cycle(l + 1, L["P"].T @ (b - A @ x))
        for _ in range(self.post):
            x = x + w * (b - A @ x)
        return x

    def ldiv(self, v):
        return self.cycle(0, np.asarray(v, np.float64))


def relerr(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0


@pytest.mark.parametrize("name,theta", rs.GRAPH_CASES)
def test_model_against_the_scipy_restatement(model, graphs, name, theta):
    """max_coarse = 1: every level with more than one unknown is split"""
    csc = graphs[name]
    n = len(csc[0]) - 1
    with np.errstate(all="ignore"):
        M = rs.RSAMGModel(model, csc, max_coarse=1, theta=theta)
        R = ScipyRS(scipy_of(csc), theta=theta, max_coarse=1)
    assert [L.n for L in M.levels] == [L["A"].shape[0] for L in R.levels], name
    for L, Q in zip(M.levels, R.levels):
        assert (L.cf is None) == (Q["cf"] is None)
        if L.cf is not None:
            assert np.array_equal(L.cf, Q["cf"]) and L.rounds == Q["rounds"], name
        assert (L.P is None) == (Q["P"] is None)
        if L.P is not None:
            assert relerr(am.dense_of(L.n, L.A), Q["A"]) <= 1e-12
            Pd = np.zeros((L.n, L.nc))
            cp, rv, nz = L.P
            for j in range(L.nc):
                Pd[rv[cp[j] - 1:cp[j + 1] - 1] - 1, j] = nz[cp[j] - 1:cp[j + 1] - 1]
            assert relerr(Pd, Q["P"]) <= 1e-12, name
    print(name, theta, "levels", [L.n for L in M.levels], "rounds", [L.rounds for L in M.levels])
    if n > 1:                                                                 # the splitting reaches one unknown, in few rounds
        assert M.levels[0].cf is not None and M.levels[-1].n == 1 and max(L.rounds for L in M.levels) <= 6
    v = np.random.default_rng(5).standard_normal(n)
    with np.errstate(all="ignore"):
        u = M.ldiv(v)
    assert np.isfinite(u).all()
    assert relerr(u, R.ldiv(v)) <= 1e-12, name


@pytest.mark.parametrize("kw", [{}, {"presweeps": 2, "postsweeps": 2}, {"presweeps": 3, "postsweeps": 1}, {"max_levels": 2},
                                {"theta": 0.5}])
def test_ldiv_with_the_defaults_against_the_scipy_restatement(model, graphs, kw):
    for name in ("fd33x31", "convdiff_pe50", "posmix", "path200"):
        csc = graphs[name]
        M = rs.RSAMGModel(model, csc, **kw)
        R = ScipyRS(scipy_of(csc), **kw)
        assert [L.n for L in M.levels] == [L["A"].shape[0] for L in R.levels] and len(M.levels) >= 2
        v = np.random.default_rng(6).standard_normal(M.n)
        assert relerr(M.ldiv(v), R.ldiv(v)) <= 1e-12, (name, kw)


@pytest.mark.parametrize("name,theta", rs.GRAPH_CASES)
def test_every_f_point_with_dependences_has_a_c_point_among_them(model, graphs, name, theta):
    csc = graphs[name]
    cp, rv, _ = csc
    n = len(cp) - 1
    cf, nc, rounds = model.rs_split(csc, theta)
    dep = model.rs_strength(csc, theta).astype(bool)
    cols = np.repeat(np.arange(n), np.diff(cp))
    rows = rv - 1
    ns = np.bincount(rows[dep], minlength=n)                                    # |S_i|
    nsc = np.bincount(rows[dep & (cf[cols] >= 0)], minlength=n)                 # |S_i & C|
    assert np.array_equal(cf == -2, ns == 0), name                             # F without interpolation <=> an empty S_i
    assert np.all(nsc[cf == -1] >= 1), name
    assert np.array_equal(cf[cf >= 0], np.arange(nc)) and (rounds == 0) == bool(np.all(ns == 0))


def test_strength_is_decided_per_row(model):
    # row 0: |-4| is the largest, theta*m = 1: -1 is strong exactly at the boundary, -0.5 is weak; row 1 depends on 0 although 0 does
    # not depend on it the same way; a stored zero, a -0.0 and a NaN are never strong, and a NaN is never the largest
    dense = np.array([[9.0, -4.0, -1.0, -0.5, 0.0], [-0.5, 9.0, 0.0, 0.0, -0.0], [-8.0, -1.9, 9.0, np.nan, 0.0],
                      [np.nan, 0.0, 0.0, 9.0, 0.0], [0.0, 0.0, 0.0, 0.0, 9.0]])
    n = 5
    cp = 1 + n * np.arange(n + 1, dtype=np.int64)
    rv = np.tile(np.arange(1, n + 1, dtype=np.int64), n)
    full = (cp, rv, np.ascontiguousarray(dense.T).reshape(-1))
    dep = model.rs_strength(full, 0.25).reshape(n, n).T                         # dep[i, j]
    want = np.array([[0, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    assert np.array_equal(dep, want)
    cf, nc, rounds = model.rs_split(full, 0.25)
    assert list(cf[3:]) == [-2, -2] and rounds >= 1 and nc >= 1


def test_both_branches_of_the_positive_part_occur_on_posmix(model, graphs):
    csc = graphs["posmix"]
    cp, rv, nz = csc
    n = len(cp) - 1
    off = (rv - 1) != np.repeat(np.arange(n), np.diff(cp))
    frac = np.sum(off & (nz > 0)) / np.sum(off)
    assert 0.1 < frac < 0.3
    S = scipy_of(csc)
    assert abs(S - S.T).max() > 0                                                # the positive pairs are unequal
    without, with_c = rs.positive_branches(model, csc, rs.THETA)
    assert without >= 1 and with_c >= 1, (without, with_c)


def test_entry_points_exist_without_a_gpu(esp):
    hdr = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    for name in ["esp_precon_rsamg_create", "esp_precon_amg_coarsening", "esp_precon_amg_splitting"]:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in esp._lib.SIGNATURES
        assert hasattr(esp._lib.load(), name)
    assert re.search(r"#define\s+ESP_AMG_COARSEN_SA\s+0\b", hdr) and esp.ESP_AMG_COARSEN_SA == 0
    assert re.search(r"#define\s+ESP_AMG_COARSEN_RS\s+1\b", hdr) and esp.ESP_AMG_COARSEN_RS == 1
    assert issubclass(esp.RS_AMGPreconditioner, esp.AMGPreconditioner) and esp.RS_AMGPreconditioner is not esp.AMGPreconditioner
    assert esp.SA_AMGPreconditioner is esp.AMGPreconditioner
    assert isinstance(esp.AMGPreconditioner.coarsening, property)
