"""Model of AMGPreconditioner (include/esparse_hip.h, esp_precon_amg_create; test infrastructure).  tests/amg_model.c is the
normative restatement of the new pieces -- strength, the Luby rounds and joining passes of the aggregation, Gauss-Jordan, the
sweeps and the V-cycle; the algebra between them is composed, by import, from the existing models: Diagonal scaling, A*B and A+B
from matops_modellib.Model, transpose and opnorm from linalg_modellib.Model, mul, dot and the solver loops from cg_modellib /
bicgstabl_modellib (through block_precon_modellib, whose cg, bicgstabl and simple! loops take any object with an ldiv).
Built with gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import block_precon_modellib
import linalg_modellib
import matops_modellib
from block_precon_modellib import RELTOL  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "amg_model.c")
DENSE_MAX = 512


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _csc(csc):
    cp, rv, nz = csc
    return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)


class Model:
    """amg_model.c's library beside the existing models it is composed with"""

    def __init__(self, outdir):
        so = os.path.join(str(outdir), "amg_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        L.model_amg_check.argtypes = [i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]
        L.model_amg_check.restype = None
        L.model_amg_strength.argtypes = [i64, vp, vp, vp, f64, vp]
        L.model_amg_strength.restype = None
        L.model_amg_aggregate.argtypes = [i64, vp, vp, vp, vp, C.POINTER(i32), vp]
        L.model_amg_aggregate.restype = i64
        L.model_amg_gauss_jordan.argtypes = [i64, vp, vp]
        L.model_amg_gauss_jordan.restype = None
        L.model_amg_cycle.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
        L.model_amg_cycle.restype = None
        self.L = L
        self.matops = matops_modellib.Model(outdir)
        self.linalg = linalg_modellib.Model(outdir)
        self.krylov = block_precon_modellib.Model(outdir)   # mul, dot, gamma

    # -- the pieces of amg_model.c
    def check(self, csc):
        """(smallest 1-based column without a stored diagonal or 0, smallest 1-based column with an unmatched entry or 0)"""
        cp, rv, _ = _csc(csc)
        a, b = C.c_int64(), C.c_int64()
        self.L.model_amg_check(len(cp) - 1, _p(cp), _p(rv), C.byref(a), C.byref(b))
        return a.value, b.value

    def strength(self, csc, theta):
        cp, rv, nz = _csc(csc)
        out = np.zeros(max(len(rv), 1), np.uint8)
        self.L.model_amg_strength(len(cp) - 1, _p(cp), _p(rv), _p(nz), float(theta), _p(out))
        return out[:len(rv)]

    def aggregate(self, csc, strong):
        """-> (agg (0-based, n), number of aggregates, Luby rounds, state (1 root, 2 excluded))"""
        cp, rv, _ = _csc(csc)
        n = len(cp) - 1
        strong = np.ascontiguousarray(np.concatenate([strong, np.zeros(1, np.uint8)]), np.uint8)
        agg = np.empty(max(n, 1), np.int64)
        state = np.empty(max(n, 1), np.uint8)
        rounds = C.c_int32()
        nc = self.L.model_amg_aggregate(n, _p(cp), _p(rv), _p(strong), _p(agg), C.byref(rounds), _p(state))
        return agg[:n].copy(), int(nc), rounds.value, state[:n].copy()

    def gauss_jordan(self, a):
        a = np.ascontiguousarray(a, np.float64)
        n = a.shape[0]
        inv = np.empty((n, n), np.float64)
        self.L.model_amg_gauss_jordan(n, _p(a), _p(inv))
        return inv

    # -- the algebra of the existing models
    def opnorm_inf(self, n, csc):
        """opnorm(A, Inf) of a square matrix, branch by branch as include/esparse_hip.h states it"""
        cp, rv, nz = _csc(csc)
        if n == 0:
            return 0.0
        if n == 1:
            return float(np.sum(np.abs(nz))) if len(nz) else 0.0   # (one value: its magnitude)
        if len(nz) == 0:
            return 0.0
        return self.linalg.opnorm_general(n, (cp, rv, nz), math.inf)


def dense_of(n, csc):
    cp, rv, nz = csc
    a = np.zeros((n, n))
    for j in range(n):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            a[rv[k] - 1, j] = nz[k]
    return a


def tentative(n, nc, agg):
    """T (n x nc) with T[i, agg(i)] = 1.0: every column's rows ascending"""
    order = np.argsort(agg, kind="stable")
    counts = np.bincount(agg, minlength=nc) if n else np.zeros(nc, np.int64)
    cp = np.ones(nc + 1, np.int64)
    np.cumsum(counts, out=cp[1:])
    cp[1:] += 1
    return cp, (order + 1).astype(np.int64), np.ones(n, np.float64)


class Level:
    def __init__(self, n, A):
        self.n, self.A = n, A
        self.P = self.w = self.agg = self.state = None
        self.rho, self.rounds, self.nc = 0.0, 0, 0


class AMGModel:
    """the hierarchy of a matrix given as host CSC arrays (update! at construction), ldiv, and the solvers with it"""

    def __init__(self, model, csc, max_levels=10, max_coarse=64, presweeps=1, postsweeps=1, theta=0.0):
        self.m = model.krylov                      # (what block_precon_modellib's solver loops call: mul, dot, gamma)
        self.model = model
        self.csc = tuple(np.array(a, copy=True) for a in _csc(csc))
        self.n = len(self.csc[0]) - 1
        self.pre, self.post = presweeps, postsweeps
        assert model.check(self.csc) == (0, 0)
        mo, la = model.matops, model.linalg
        self.levels, self.inv = [], None
        A = self.csc
        n = self.n
        while True:
            L = Level(n, A)
            self.levels.append(L)
            cp, rv, nz = A
            with np.errstate(all="ignore"):
                diag = np.zeros(n)
                for j in range(n):
                    for k in range(cp[j] - 1, cp[j + 1] - 1):
                        if rv[k] - 1 == j:
                            diag[j] = nz[k]
                dinv = np.float64(1.0) / diag                       # invdiag as esp_jacobi_setup gives it
                L.rho = float(model.opnorm_inf(n, mo.diag_scale(A, dinv, 0)))
                omega = np.float64(4.0 / 3.0) / np.float64(L.rho)
                L.w = omega * dinv
            coarsest = n <= max_coarse or len(self.levels) == max_levels
            if not coarsest:
                strong = model.strength(A, theta)
                L.strong = strong
                L.agg, L.nc, L.rounds, L.state = model.aggregate(A, strong)
                assert L.agg.min() >= 0
                coarsest = L.nc == n
            if coarsest:
                if n <= DENSE_MAX:
                    with np.errstate(all="ignore"):
                        self.inv = model.gauss_jordan(dense_of(n, A))
                break
            nc = L.nc
            T = tentative(n, nc, L.agg)
            DAT = mo.matmul(n, mo.diag_scale(A, -L.w, 0), T)
            L.P = mo.add(T, DAT)
            AP = mo.matmul(n, A, L.P)
            PT = la.transpose(n, L.P)
            A = mo.matmul(nc, PT, AP)
            n = nc

    def ldiv(self, v):
        v = np.ascontiguousarray(v, np.float64)
        nlev = len(self.levels)
        keep = []

        def ptrs(get):
            arr = (C.c_void_p * nlev)()
            for l, L in enumerate(self.levels):
                a = get(L)
                if a is not None:
                    a = np.ascontiguousarray(a)
                    keep.append(a)
                    arr[l] = a.ctypes.data
            return arr
        ns = np.array([L.n for L in self.levels], np.int64)
        acp, arv, anz = ptrs(lambda L: L.A[0]), ptrs(lambda L: L.A[1]), ptrs(lambda L: L.A[2])
        pcp = ptrs(lambda L: L.P[0] if L.P else None)
        prv = ptrs(lambda L: L.P[1] if L.P else None)
        pnz = ptrs(lambda L: L.P[2] if L.P else None)
        w = ptrs(lambda L: L.w)
        u = np.empty(max(self.n, 1), np.float64)
        inv = np.ascontiguousarray(self.inv) if self.inv is not None else None
        self.model.L.model_amg_cycle(nlev, _p(ns), acp, arv, anz, pcp, prv, pnz, w, _p(inv), self.pre, self.post, _p(v), _p(u))
        return u[:self.n].copy()

    def mul(self, x):
        return self.m.mul(self.csc, x)

    def norm(self, r):
        return float(np.sqrt(self.m.dot(r, r)))

    # the solver loops of include/esparse_hip.h as block_precon_modellib restates them over an ldiv
    cg = block_precon_modellib.BlockModel.cg
    bicgstabl = block_precon_modellib.BlockModel.bicgstabl
    simple = block_precon_modellib.BlockModel.simple
    simple_norm = staticmethod(block_precon_modellib.BlockModel.simple_norm)


def operator_complexity(levels):
    return sum(len(L.A[1]) for L in levels) / max(len(levels[0].A[1]), 1)


# ---- the graphs of the aggregation tests, as Julia CSC arrays (every pattern structurally symmetric, every diagonal stored) ----
def csc_of_scipy(S):
    import scipy.sparse as sp
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def path_graph(n):
    """tridiag(-1, 2 + a little, -1); n = 1: the single entry"""
    import scipy.sparse as sp
    if n == 1:
        return csc_of_scipy(sp.csc_matrix(np.array([[2.0]])))
    return csc_of_scipy(sp.diags([-np.ones(n - 1), 2.0 + 0.01 * np.arange(n), -np.ones(n - 1)], [-1, 0, 1]))


def star_graph(deg, hub=0):
    """a hub joined to deg leaves (n = deg + 1): the hub's column holds deg + 1 entries"""
    import scipy.sparse as sp
    n = deg + 1
    S = sp.lil_matrix((n, n))
    for i in range(n):
        S[i, i] = 2.0 + 0.001 * i
    S[hub, hub] = deg + 1.0
    for i in range(n):
        if i != hub:
            S[i, hub] = -1.0 - 0.001 * i
            S[hub, i] = -1.0 - 0.002 * i
    return csc_of_scipy(S)


def dirichlet_like(csc, rows, isolated):
    """rows: their off-diagonal entries become stored zeros, the diagonal 1.0 (the columns keep their values); isolated: row AND
    column off-diagonals become stored zeros -- the pattern is unchanged"""
    cp, rv, nz = (np.array(a, copy=True) for a in csc)
    n = len(cp) - 1
    for j in range(n):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            i = rv[k] - 1
            if i == j:
                if i in rows:
                    nz[k] = 1.0
            elif i in rows or i in isolated or j in isolated:
                nz[k] = 0.0
    return cp, rv, nz


def dense_block(n, seed=5):
    """a full symmetric n x n matrix, diagonally dominant"""
    rng = np.random.default_rng(seed)
    M = -rng.random((n, n))
    M = 0.5 * (M + M.T)
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, 1.0 - M.sum(axis=1))
    cp = 1 + n * np.arange(n + 1, dtype=np.int64)
    rv = np.tile(np.arange(1, n + 1, dtype=np.int64), n)
    return cp, rv, np.ascontiguousarray(M.T).reshape(-1)


def convdiff(nx, ny, nz, pe, seed=1):
    from bicgstabl_modellib import convdiff_triplets, csc_arrays
    return csc_arrays(nx * ny * nz, *convdiff_triplets(nx, ny, nz, pe, seed))


EMPTY = (np.ones(1, np.int64), np.zeros(0, np.int64), np.zeros(0))


def graphs(fd):
    """name -> (CSC arrays, theta): the graphs of the aggregation tests, on the CPU and on the device; fd(nx, ny, nz) gives the
    CSC arrays of an fdrand matrix"""
    g = {"n0": (EMPTY, 0.0), "n1": (path_graph(1), 0.0), "n2": (path_graph(2), 0.0)}
    for n in (3, 5, 200):
        g["path%d" % n] = (path_graph(n), 0.0)
    g["fd5x5x5"] = (fd(5, 5, 5), 0.0)
    g["fd33x31"] = (fd(33, 31, 1), 0.0)
    for d in (33, 64, 65, 130, 31, 32, 63):
        g["star%d" % d] = (star_graph(d, hub=d // 2), 0.0)
    g["dirichlet"] = (dirichlet_like(fd(9, 8, 1), rows={0, 13, 14, 40}, isolated={5, 30, 71}), 0.0)
    g["dense70"] = (dense_block(70), 0.0)
    g["convdiff_t0"] = (convdiff(6, 5, 4, 4.0), 0.0)
    g["convdiff_t025"] = (convdiff(6, 5, 4, 4.0), 0.25)
    return g


GRAPH_NAMES = ["n0", "n1", "n2", "path3", "path5", "path200", "fd5x5x5", "fd33x31", "star33", "star64", "star65", "star130",
               "star31", "star32", "star63",
               "dirichlet", "dense70", "convdiff_t0", "convdiff_t025"]
