"""ctypes binding of tests/iluam_model.c (test infrastructure): the reference's iluAM / ldiv! / simple! with
ILUAMPreconditioner restated as literal loops, plus the same work in a caller-supplied level order; and a NumPy
restatement of the three level schedules.  Built with gcc -O1 -ffp-contract=off (together with precon_model.c, whose mul!
and norm simple! uses) into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "iluam_model.c"), os.path.join(HERE, "precon_model.c")]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "iluam_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so] + SRCS + ["-lm"])
        L = C.CDLL(so)
        i64, f64, vp = C.c_int64, C.c_double, C.c_void_p
        L.model_iluam_diag.argtypes = [i64, vp, vp, vp]
        L.model_iluam_diag.restype = i64
        L.model_iluam_factor.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_factor.restype = None
        L.model_iluam_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_iluam_ldiv.restype = None
        L.model_iluam_ldiv_rows.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.model_iluam_ldiv_rows.restype = None
        L.model_iluam_simple.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, i64, f64, f64, vp]
        L.model_iluam_simple.restype = i64
        self.L = L

    @staticmethod
    def _csc(csc):
        cp, rv, nz = csc
        return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)

    def factor(self, csc, order=None):
        """iluAM(A) -> (nzval of the factorization, diag); order: 1-based column numbers in the order to run them"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        diag = np.zeros(max(n, 1), np.int64)
        missing = self.L.model_iluam_diag(n, _p(cp), _p(rv), _p(diag))
        if missing:
            raise ValueError("column %d has no stored diagonal" % missing)
        f = nz.copy()
        order = None if order is None else np.ascontiguousarray(order, np.int64)
        self.L.model_iluam_factor(n, _p(cp), _p(rv), _p(diag), _p(f), _p(order))
        return f, diag[:n]

    def ldiv(self, csc, fval, diag, v, inplace=False, fwd=None, bwd=None):
        """ldiv!(x, ILU, v) (x === v with inplace); fwd / bwd: run as row gathers in these orders (1-based rows)"""
        cp, rv, _ = self._csc(csc)
        fval = np.ascontiguousarray(fval, np.float64)
        diag = np.ascontiguousarray(diag, np.int64)
        v = np.array(v, np.float64)
        x = v if inplace else np.empty_like(v)
        if fwd is None:
            self.L.model_iluam_ldiv(len(v), _p(cp), _p(rv), _p(fval), _p(diag), _p(v), _p(x))
        else:
            fwd = np.ascontiguousarray(fwd, np.int64)
            bwd = np.ascontiguousarray(bwd, np.int64)
            self.L.model_iluam_ldiv_rows(len(v), _p(cp), _p(rv), _p(fval), _p(diag), _p(v), _p(x), _p(fwd), _p(bwd))
        return x

    def simple(self, csc, fval, diag, b, u=None, maxiter=100, abstol=0.0, reltol=np.sqrt(np.finfo(float).eps)):
        """-> (u, history, iterations)"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        b = np.ascontiguousarray(b, np.float64)
        u = np.zeros(n) if u is None else np.array(u, np.float64)
        fval = np.ascontiguousarray(fval, np.float64)
        diag = np.ascontiguousarray(diag, np.int64)
        hist = np.empty(maxiter + 1)
        it = self.L.model_iluam_simple(n, _p(cp), _p(rv), _p(nz), _p(fval), _p(diag), _p(b), _p(u), maxiter, abstol, reltol, _p(hist))
        return u, hist[:it + 1].copy(), it


def level_schedules(cp, rv):
    """The three level schedules from the pattern alone (1-based CSC arrays), as arrays level[node]:
    columns of the factorization (column j after every column i < j with a stored (i,j)), rows of the forward solve
    (row i after every row j < i with a stored (i,j)), rows of the backward solve (... j > i)."""
    n = len(cp) - 1
    pat = sp.csc_matrix((np.ones(len(rv), np.int8), np.asarray(rv) - 1, np.asarray(cp) - 1), shape=(n, n))
    pat.sort_indices()
    csr = pat.tocsr()
    csr.sort_indices()

    def sweep(ptr, idx, nodes, before):
        lev = np.zeros(n, np.int64)
        for i in nodes:
            d = idx[ptr[i]:ptr[i + 1]]
            d = d[d < i] if before else d[d > i]
            if len(d):
                lev[i] = lev[d].max() + 1
        return lev

    return (sweep(pat.indptr, pat.indices, range(n), True),
            sweep(csr.indptr, csr.indices, range(n), True),
            sweep(csr.indptr, csr.indices, range(n - 1, -1, -1), False))


def level_order(lev, reverse_inside=False):
    """1-based node numbers sorted by level, ascending inside a level (or descending: any order inside a level is legal)"""
    n = len(lev)
    idx = np.arange(n)
    order = np.lexsort((-idx if reverse_inside else idx, lev))
    return order + 1
