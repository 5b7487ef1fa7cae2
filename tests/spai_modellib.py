"""ctypes binding of tests/spai_model.c (test infrastructure): the normative model of SPAIPreconditioner -- SPAI-0 and SPAI-1 as
plain loops -- and, around it, the preconditioner object the statement-by-statement solver models are driven with.  The
symmetrised form 0.5*(M + transpose(M)) is put together from the models of the calls the device uses (matops_model.c's A + B and
Diagonal scaling; the transpose is a bitwise permutation); ldiv is the product in esp_mul's order (model_mul).  Built with
gcc -O1 -ffp-contract=off into a directory the caller chooses."""
import ctypes as C
import os
import subprocess

import numpy as np

import block_precon_modellib
import matops_modellib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "spai_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _csc(csc):
    cp, rv, nz = csc
    return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)


def transpose(csc):
    """copy(transpose(A)) of square Julia CSC arrays: every stored entry, bits kept, rows ascending in every column"""
    cp, rv, nz = _csc(csc)
    n = len(cp) - 1
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    order = np.lexsort((cols, rv - 1))                      # by (row of A = column of the transpose, then column of A)
    tcp = np.ones(n + 1, np.int64)
    np.cumsum(np.bincount(rv - 1, minlength=n), out=tcp[1:])
    tcp[1:] += 1
    return tcp, (cols[order] + 1).astype(np.int64), nz[order].copy()


def csc_from_columns(cols, rng):
    """Julia CSC arrays of the pattern cols (cols[j] = the stored rows of column j, 0-based), seeded values: 4 + U(0,1) on the
    diagonal, U(-1, 1) elsewhere"""
    cp, rv, nz = [1], [], []
    for j, col in enumerate(cols):
        col = sorted(set(int(r) for r in col))
        rv.extend(r + 1 for r in col)
        nz.extend(4.0 + rng.random() if r == j else rng.uniform(-1.0, 1.0) for r in col)
        cp.append(cp[-1] + len(col))
    return np.array(cp, np.int64), np.array(rv, np.int64), np.array(nz, np.float64)


def hub_columns(h):
    """n = h + 1.  Column 0, the hub, stores the h rows 1..h (no diagonal); column 1 stores 0, 1, 2; the columns 2..h store row 1
    alone.  Column 1 has q = 3 unknowns and the p = h + 1 rows 0..h: p crosses the lane strides of the ordered sum with h.  The
    hub itself has q = h unknowns over the p = 3 rows 0, 1, 2: rank-deficient, and with q*q > ESP_SPAI_WAVE_DOUBLES the workgroup
    tier's."""
    return [list(range(1, h + 1)), [0, 1, 2]] + [[1] for _ in range(2, h + 1)]


def sized_columns(p, q):
    """n = p >= q >= 2.  Column 0 stores the rows 0..q-1; the columns 1..q-1 their diagonal and, dealt round-robin, the rows
    q..p-1; the columns q..p-1 their diagonal alone.  Column 0 has exactly q unknowns and p rows."""
    cols = [list(range(q))] + [[j] for j in range(1, p)]
    for t, r in enumerate(range(q, p)):
        cols[1 + t % (q - 1)].append(r)
    return cols


def too_large_columns(rows):
    """n = rows.  Column 0 stores row 1 alone, column 1 stores every row, the others are empty: column 0 has q = 1 unknown over
    p = rows rows"""
    return [[1], list(range(rows))] + [[] for _ in range(2, rows)]


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "spai_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_spai0.argtypes = [i64, vp, vp, vp, vp]
        L.model_spai0.restype = None
        L.model_spai1.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_spai1.restype = i64
        self.L = L
        self.solver = block_precon_modellib.Model(outdir)   # mul, dot and the solvers' C parts
        self.matops = matops_modellib.Model(outdir)

    def spai0(self, csc):
        cp, rv, nz = _csc(csc)
        n = len(cp) - 1
        d = np.empty(n, np.float64)
        self.L.model_spai0(n, _p(cp), _p(rv), _p(nz), _p(d))
        return d

    def spai1(self, csc):
        """-> (m: nnz values in A's position order, p of every column, (max p, max q, max p*q))"""
        cp, rv, nz = _csc(csc)
        n = len(cp) - 1
        m = np.empty(len(nz), np.float64)
        pcol, stats = np.zeros(n, np.int64), np.zeros(4, np.int64)
        assert self.L.model_spai1(n, _p(cp), _p(rv), _p(nz), _p(m), _p(pcol), _p(stats)) == 0
        return m, pcol, tuple(int(x) for x in stats[:3])

    def precon(self, csc, order=1, symmetric=False):
        return SpaiPrecon(self, csc, order, symmetric)


class SolverModel(block_precon_modellib.BlockModel):
    """BlockModel's statement-by-statement cg, bicgstabl and simple! (and gmres_modellib's gmres_cb) driven with a model
    preconditioner's ldiv -- an object with .csc, .n and .ldiv -- and A's mul"""

    def __init__(self, lib, precon):
        self.m, self.P, self.csc, self.n = lib, precon, precon.csc, precon.n

    def ldiv(self, v):
        return self.P.ldiv(np.ascontiguousarray(v, np.float64))


class JacobiPrecon:
    """jacobi(A) for the comparison of iteration counts: invdiag[j] = 1 / A[j,j], ldiv! u = invdiag .* v"""

    def __init__(self, csc):
        self.csc = tuple(np.array(a, copy=True) for a in _csc(csc))
        cp, rv, nz = self.csc
        self.n = len(cp) - 1
        d = np.zeros(self.n)
        for j in range(self.n):
            for e in range(cp[j] - 1, cp[j + 1] - 1):
                if rv[e] - 1 == j:
                    d[j] = nz[e]
        with np.errstate(all="ignore"):
            self.inv = 1.0 / d

    def ldiv(self, v):
        return self.inv * v


class SpaiPrecon:
    """the model's preconditioner: .diag (order 0) or .M (order 1: the applied matrix as Julia CSC arrays), .raw (M before the
    symmetrisation), .pcol, .stats, ldiv; .csc and .n for the solver models"""

    def __init__(self, model, csc, order, symmetric):
        assert order in (0, 1) and not (symmetric and order == 0)
        self.m, self.order, self.symmetric = model, order, symmetric
        self.csc = tuple(np.array(a, copy=True) for a in _csc(csc))
        self.n = len(self.csc[0]) - 1
        if order == 0:
            self.diag = model.spai0(self.csc)
            return
        vals, self.pcol, self.stats = model.spai1(self.csc)
        self.raw = (self.csc[0].copy(), self.csc[1].copy(), vals)
        self.M = self.raw
        if symmetric:
            s = model.matops.add(self.raw, transpose(self.raw))
            self.M = model.matops.diag_scale(s, np.full(self.n, 0.5), 0)

    def factor(self):
        return self.diag if self.order == 0 else self.M[2]

    def ldiv(self, v, inplace=False):
        v = np.ascontiguousarray(v, np.float64)
        if self.order == 0:
            u = np.empty(self.n)
            for i in range(self.n):
                u[i] = self.diag[i] * v[i]
        else:
            u = self.m.solver.mul(self.M, v) if self.n else np.empty(0)
        if inplace:
            v[:] = u
            return v
        return u
