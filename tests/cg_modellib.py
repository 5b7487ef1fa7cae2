"""ctypes binding of tests/cg_model.c (test infrastructure): preconditioned conjugate gradients as esp_cg states them, as
literal loops, with the device's summation shape restated on its own.  cg_model.c includes precon_model.c and iluam_model.c
(ldiv! and mul! are theirs).  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp
directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cg_model.c")
KIND_IDENTITY, KIND_JACOBI, KIND_ILU0, KIND_ILUAM = -1, 0, 1, 2
KINDS = {"identity": KIND_IDENTITY, "jacobi": KIND_JACOBI, "ilu0": KIND_ILU0, "iluam": KIND_ILUAM}
RELTOL = float(np.sqrt(np.finfo(np.float64).eps))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Precon:
    """what the model's ldiv! needs: kind, diag (invdiag / xdiag), idiag (ILU0's idiag / ILUAM's diag), fval (ILUAM)"""

    def __init__(self, kind, diag=None, idiag=None, fval=None):
        self.kind, self.diag, self.idiag, self.fval = kind, diag, idiag, fval


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "cg_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        L.model_cg_dot.argtypes = [i64, vp, vp]
        L.model_cg_dot.restype = f64
        L.model_cg.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, f64, f64, vp, C.POINTER(i32)]
        L.model_cg.restype = i64
        L.model_jacobi_ldiv.argtypes = [i64, vp, vp, vp]
        L.model_ilu0_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_iluam_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_mul.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_diag.argtypes = [i64, vp, vp, vp]
        L.model_iluam_diag.restype = i64
        L.model_iluam_factor.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_factor.restype = None
        self.L = L

    @staticmethod
    def _csc(csc):
        cp, rv, nz = csc
        return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)

    def dot(self, a, b):
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        return self.L.model_cg_dot(len(a), _p(a), _p(b))

    def mul(self, csc, x):
        cp, rv, nz = self._csc(csc)
        x = np.ascontiguousarray(x, np.float64)
        r = np.empty_like(x)
        self.L.model_mul(len(x), _p(cp), _p(rv), _p(nz), _p(x), _p(r))
        return r

    def precon(self, kind, csc, orc):
        """the reference's factorization of the CSC arrays: jacobi(A) / ilu0(A) from the oracle, iluAM(A) from iluam_model.c"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        if kind == "identity":
            return Precon(KIND_IDENTITY)
        if kind == "jacobi":
            return Precon(KIND_JACOBI, diag=np.ascontiguousarray(orc.CSC(n, n, cp, rv, nz).jacobi(), np.float64))
        if kind == "ilu0":
            xd, idg = orc.CSC(n, n, cp, rv, nz).ilu0()
            return Precon(KIND_ILU0, diag=np.ascontiguousarray(xd, np.float64), idiag=np.ascontiguousarray(idg, np.int64))
        assert kind == "iluam"
        diag = np.zeros(max(n, 1), np.int64)
        missing = self.L.model_iluam_diag(n, _p(cp), _p(rv), _p(diag))
        assert missing == 0
        f = nz.copy()
        self.L.model_iluam_factor(n, _p(cp), _p(rv), _p(diag), _p(f), None)
        return Precon(KIND_ILUAM, idiag=diag, fval=f)

    def ldiv(self, P, csc, v):
        """Pl \\ v (a LinearOperator for scipy's cg)"""
        cp, rv, nz = self._csc(csc)
        v = np.ascontiguousarray(v, np.float64)
        n = len(v)
        u = np.empty_like(v)
        if P.kind == KIND_IDENTITY:
            u[:] = v
        elif P.kind == KIND_JACOBI:
            self.L.model_jacobi_ldiv(n, _p(P.diag), _p(v), _p(u))
        elif P.kind == KIND_ILU0:
            self.L.model_ilu0_ldiv(n, _p(cp), _p(rv), _p(nz), _p(P.diag), _p(P.idiag), _p(v), _p(u))
        else:
            self.L.model_iluam_ldiv(n, _p(cp), _p(rv), _p(P.fval), _p(P.idiag), _p(v), _p(u))
        return u

    def cg(self, P, csc, b, x=None, maxiter=None, abstol=0.0, reltol=RELTOL):
        """-> (x, history (iterations + 1 norms), iterations, converged); x = None: cg from zeros, else cg! on a copy"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        b = np.ascontiguousarray(b, np.float64)
        zero = 1 if x is None else 0
        x = np.zeros(n) if x is None else np.array(x, np.float64)
        maxiter = n if maxiter is None else maxiter
        hist = np.empty(maxiter + 1)
        conv = C.c_int32()
        it = self.L.model_cg(P.kind, n, _p(cp), _p(rv), _p(nz), _p(P.diag), _p(P.idiag), _p(P.fval), _p(b), _p(x), zero, maxiter,
                             abstol, reltol, _p(hist), C.byref(conv))
        return x, hist[:it + 1].copy(), it, bool(conv.value)
