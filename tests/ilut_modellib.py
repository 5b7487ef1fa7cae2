"""ctypes binding of tests/ilut_model.c (test infrastructure): ILUTPreconditioner's construction and warm update, entry by entry,
with the update state; the application is iluam_modellib's ldiv! over (S, F).  Beside it a dense NumPy restatement of the same
algorithm (another summation order: np.dot), which tests/test_ilut_model.py compares the model with.  Built with
gcc -O1 -ffp-contract=off into a directory the caller chooses."""
import ctypes as C
import os
import subprocess

import numpy as np

import iluam_modellib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ilut_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class FillRefused(Exception):
    """the max_fill guard: step (0-based), nnz(C), the limit (int64)(max_fill * nnz(A))"""

    def __init__(self, step, nnz_c, limit):
        super().__init__("step %d: nnz(C) = %d > %d" % (step, nnz_c, limit))
        self.step, self.nnz_c, self.limit = step, nnz_c, limit


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "ilut_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp = C.c_int64, C.c_double, C.c_void_p
        L.model_ilut.argtypes = [i64, vp, vp, vp, f64, i64, i64, f64, i64, vp, vp, vp, vp, vp]
        L.model_ilut.restype = i64
        L.model_ilut_sweeps.argtypes = [i64, vp, vp, vp, vp, vp, vp, i64]
        L.model_ilut_sweeps.restype = None
        self.L = L
        self.iluam = iluam_modellib.Model(outdir)

    def precon(self, csc, droptol=1e-3, steps=3, sweeps=3, max_fill=32.0, keep_pattern=False):
        return IlutPrecon(self, csc, droptol, steps, sweeps, max_fill, keep_pattern)


def _csc(csc):
    return tuple(np.array(a, dtype=t, copy=True) for a, t in zip(csc, (np.int64, np.int64, np.float64)))


class IlutPrecon:
    """the model's preconditioner with its update state: .S = (colptr, rowval), .F, .stats (nnz(C), nnz(S) per step), .sweeps_run;
    update(csc) is update! for A's new arrays; ldiv is iluam_model.c's over (S, F); .csc / .n: what the solver models read"""

    def __init__(self, model, csc, droptol, steps, sweeps, max_fill, keep_pattern):
        self.m = model
        self.par = (float(droptol), int(steps), int(sweeps), float(max_fill))
        self.keep_pattern = bool(keep_pattern)
        self.S = None
        self._construct(_csc(csc))

    def _construct(self, csc):
        cp, rv, nz = csc
        n = len(cp) - 1
        tau, steps, sweeps, max_fill = self.par
        nnz = len(rv)
        cap = max(min(int(max_fill * nnz), n * n), nnz, 1)
        scp, srv, f = np.empty(n + 1, np.int64), np.empty(cap, np.int64), np.empty(cap, np.float64)
        stats, info = np.zeros(2 * max(steps, 1), np.int64), np.zeros(3, np.int64)
        r = self.m.L.model_ilut(n, _p(cp), _p(rv), _p(nz), tau, steps, sweeps, max_fill, cap, _p(scp), _p(srv), _p(f), _p(stats), _p(info))
        if r == -1:
            raise ValueError("column %d has no stored diagonal" % info[0])
        if r == -2:
            raise FillRefused(int(info[0]), int(info[1]), int(info[2]))      # (the state of the last good update stays)
        assert r >= 0, r
        self.csc, self.n = csc, n
        self.S, self.F = (scp, srv[:r].copy()), f[:r].copy()
        self.stats = [(int(stats[2 * t]), int(stats[2 * t + 1])) for t in range(steps)]
        self.sweeps_run = (2 * steps if steps else 1) * sweeps
        self.diag = np.array([scp[j] + int(np.searchsorted(srv[scp[j] - 1:scp[j + 1] - 1], j + 1)) for j in range(n)], np.int64)

    def update(self, csc):
        csc = _csc(csc)
        same = np.array_equal(csc[0], self.csc[0]) and np.array_equal(csc[1], self.csc[1])
        if not (same and self.keep_pattern):
            self._construct(csc)
            return self
        self.csc = csc
        self.sweep(self.par[2])
        self.sweeps_run = self.par[2]
        return self

    def sweep(self, count):
        """`count` more sweeps on the kept pattern, from the current F and A's current values"""
        cp, rv, nz = self.csc
        self.m.L.model_ilut_sweeps(self.n, _p(cp), _p(rv), _p(nz), _p(self.S[0]), _p(self.S[1]), _p(self.F), int(count))
        return self

    @property
    def B(self):
        """(S, F) as CSC arrays: what iluam_modellib's ldiv and the level analysis read"""
        return self.S[0], self.S[1], self.F

    def ldiv(self, v, inplace=False):
        return self.m.iluam.ldiv(self.B, self.F, self.diag, v, inplace=inplace)


# ---- the dense restatement ---------------------------------------------------------------------------------------------------------
def dense_of(csc):
    cp, rv, nz = csc
    n = len(cp) - 1
    A, P = np.zeros((n, n)), np.zeros((n, n), bool)
    for j in range(n):
        for q in range(cp[j] - 1, cp[j + 1] - 1):
            A[rv[q] - 1, j] = nz[q]
            P[rv[q] - 1, j] = True
    return A, P


def dense_sweep(A, P, F):
    """one synchronous sweep, the sums by np.dot over the masked row and column (not the model's order)"""
    n = len(A)
    L, U = np.where(np.tril(P, -1), F, 0.0), np.where(np.triu(P), F, 0.0)
    G = np.zeros_like(F)
    for i, j in zip(*np.nonzero(P)):
        m = min(i, j)
        r = A[i, j] - np.dot(L[i, :m], U[:m, j])
        G[i, j] = r / F[j, j] if i > j else r
    return G


def dense_ilut(csc, droptol, steps, sweeps):
    """-> (pattern, F) as dense arrays"""
    A, P = dense_of(csc)
    n = len(A)
    d = np.diag(A)
    F = np.where(np.tril(P, -1), A / d[None, :], A)
    F = np.where(P, F, 0.0)

    def run(P, F):
        for _ in range(sweeps):
            F = dense_sweep(A, P, F)
        return F
    if steps == 0:
        return P, run(P, F)
    for _ in range(steps):
        Lp = np.tril(P).astype(np.int64)
        Up = np.triu(P).astype(np.int64)
        Cp = (Lp @ Up) > 0
        F = run(Cp, F)
        dd = np.abs(np.diag(F))
        keep = Cp & ~((np.tril(np.ones((n, n), bool), -1) & (np.abs(F) < droptol)) |
                      (np.triu(np.ones((n, n), bool), 1) & (np.abs(F) < droptol * dd[:, None])))
        P = keep
        F = run(P, np.where(P, F, 0.0))
    return P, F


def dense_from(S, F, n):
    cp, rv = S
    D, P = np.zeros((n, n)), np.zeros((n, n), bool)
    for j in range(n):
        for q in range(cp[j] - 1, cp[j + 1] - 1):
            D[rv[q] - 1, j] = F[q]
            P[rv[q] - 1, j] = True
    return P, D


def restricted(csc, S):
    """the matrix with A's values on S and +0.0 elsewhere, as CSC arrays on S"""
    cp, rv, nz = csc
    scp, srv = S
    out = np.zeros(len(srv))
    for j in range(len(cp) - 1):
        rows = rv[cp[j] - 1:cp[j + 1] - 1]
        for q in range(scp[j] - 1, scp[j + 1] - 1):
            k = np.searchsorted(rows, srv[q])
            if k < len(rows) and rows[k] == srv[q]:
                out[q] = nz[cp[j] - 1 + k]
    return scp, srv, out
