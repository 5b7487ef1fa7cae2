"""ctypes binding of tests/precon_model.c (test infrastructure): the reference's ldiv! / mul! / simple! restated as literal
loops.  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "precon_model.c")
KIND_JACOBI, KIND_ILU0 = 0, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "precon_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        L.model_jacobi_ldiv.argtypes = [i64, vp, vp, vp]
        L.model_ilu0_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_mul.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_norm.argtypes = [i64, vp]
        L.model_norm.restype = f64
        L.model_simple.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, i64, f64, f64, vp]
        L.model_simple.restype = i64
        self.L = L

    @staticmethod
    def _csc(csc):
        cp, rv, nz = (np.ascontiguousarray(a) for a in csc)
        return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)

    def jacobi_ldiv(self, invdiag, v):
        invdiag = np.ascontiguousarray(invdiag, np.float64)
        v = np.ascontiguousarray(v, np.float64)
        u = np.empty_like(v)
        self.L.model_jacobi_ldiv(len(v), _p(invdiag), _p(v), _p(u))
        return u

    def ilu0_ldiv(self, csc, xdiag, idiag, v, inplace=False):
        cp, rv, nz = self._csc(csc)
        xdiag = np.ascontiguousarray(xdiag, np.float64)
        idiag = np.ascontiguousarray(idiag, np.int64)
        v = np.array(v, np.float64)
        u = v if inplace else np.empty_like(v)
        self.L.model_ilu0_ldiv(len(v), _p(cp), _p(rv), _p(nz), _p(xdiag), _p(idiag), _p(v), _p(u))
        return u

    def mul(self, csc, x):
        cp, rv, nz = self._csc(csc)
        x = np.ascontiguousarray(x, np.float64)
        r = np.empty_like(x)
        self.L.model_mul(len(x), _p(cp), _p(rv), _p(nz), _p(x), _p(r))
        return r

    def norm(self, x):
        x = np.ascontiguousarray(x, np.float64)
        return self.L.model_norm(len(x), _p(x))

    def simple(self, kind, csc, diag, idiag, b, u=None, maxiter=100, abstol=0.0, reltol=np.sqrt(np.finfo(float).eps)):
        """-> (u, history, iterations)"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        b = np.ascontiguousarray(b, np.float64)
        u = np.zeros(n) if u is None else np.array(u, np.float64)
        diag = np.ascontiguousarray(diag, np.float64)
        idg = np.ascontiguousarray(idiag if idiag is not None else np.zeros(n, np.int64), np.int64)
        hist = np.empty(maxiter + 1)
        it = self.L.model_simple(kind, n, _p(cp), _p(rv), _p(nz), _p(diag), _p(idg), _p(b), _p(u), maxiter, abstol, reltol,
                                 _p(hist))
        return u, hist[:it + 1].copy(), it
