"""ctypes binding of tests/gmres_model.c (test infrastructure): restarted GMRES as esp_gmres states it, as literal loops.
gmres_model.c includes cg_model.c (ldiv!, mul! and the ordered dot product are its), so this Model offers everything
cg_modellib's does (precon, mul, ldiv, dot) plus gmres (the C loops of the four point kinds) and gmres_cb (the same loop over
any object with .mul(v) and .ldiv(v): block_precon_modellib's BlockModel, amg_modellib's AMGModel).  Built with
gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

import cg_modellib
from cg_modellib import KINDS, RELTOL, Precon, _p  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gmres_model.c")
ORTH = {"mgs": 0, "cgs": 1, "dgks": 2}
RESTART_MAX = 64
APPLY = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))


class Probe(C.Structure):
    _fields_ = [("H", C.c_void_p), ("V", C.c_void_p), ("cycle_m", C.POINTER(C.c_int64)), ("restart_x", C.c_void_p),
                ("restart_it", C.c_void_p), ("cycles_cap", C.c_int64), ("cycles", C.POINTER(C.c_int64))]


class Result:
    """x, history (iters + 1 norms), iters, mvps, reorth, converged; with probe=True also H (before the rotations) and V of the
    last finished cycle, its number of columns m, and x / the iteration count after every cycle"""

    def __iter__(self):
        return iter((self.x, self.history, self.iters, self.mvps, self.reorth, self.converged))


class Model(cg_modellib.Model):
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "gmres_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        L.model_cg_dot.argtypes = [i64, vp, vp]
        L.model_cg_dot.restype = f64
        tail = [vp, vp, i32, i32, i32, i64, f64, f64, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(Probe)]
        L.model_gmres.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp] + tail
        L.model_gmres.restype = i64
        L.model_gmres_cb.argtypes = [i64, APPLY, APPLY] + tail
        L.model_gmres_cb.restype = i64
        L.model_gmres_lsq.argtypes = [i32, i32, vp, f64, vp]
        L.model_gmres_lsq.restype = None
        L.model_jacobi_ldiv.argtypes = [i64, vp, vp, vp]
        L.model_ilu0_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_iluam_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_mul.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_diag.argtypes = [i64, vp, vp, vp]
        L.model_iluam_diag.restype = i64
        L.model_iluam_factor.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_factor.restype = None
        self.L = L

    def lsq(self, H, beta):
        """y of min |beta e1 - H y| for the (m+1) x m Hessenberg matrix H: the Givens rotations and the back substitution"""
        m = H.shape[1]
        Hc = np.asfortranarray(H, np.float64).copy(order="F")
        rhs = np.zeros(m + 1)
        self.L.model_gmres_lsq(m, m + 1, _p(Hc), float(beta), _p(rhs))
        return rhs[:m].copy()

    def _run(self, call, n, b, x, restart, orth_meth, maxiter, abstol, reltol, probe):
        b = np.ascontiguousarray(b, np.float64)
        zero = 1 if x is None else 0
        x = np.zeros(n) if x is None else np.array(x, np.float64)
        restart = max(1, min(20, n)) if restart is None else restart
        maxiter = n if maxiter is None else maxiter
        hist = np.empty(maxiter + 1)
        conv, mv, re = C.c_int32(), C.c_int64(), C.c_int64()
        pr, keep = None, None
        if probe and n > 0:
            cap = maxiter // restart + 2
            keep = (np.zeros((restart, restart + 1)), np.zeros((restart + 1, n)), C.c_int64(), np.zeros((cap, n)),
                    np.zeros(cap, np.int64), C.c_int64())
            pr = Probe(keep[0].ctypes.data, keep[1].ctypes.data, C.pointer(keep[2]), keep[3].ctypes.data, keep[4].ctypes.data, cap,
                       C.pointer(keep[5]))
        it = call(_p(b), _p(x), zero, restart, ORTH[orth_meth], maxiter, abstol, reltol, _p(hist), C.byref(mv), C.byref(re),
                  C.byref(conv), C.byref(pr) if pr is not None else None)
        assert it >= 0
        r = Result()
        r.x, r.history, r.iters, r.mvps, r.reorth, r.converged = x, hist[:it + 1].copy(), it, mv.value, re.value, bool(conv.value)
        if keep is not None:
            r.m = keep[2].value
            r.H = keep[0].T[:r.m + 1, :r.m].copy()          # (column-major, leading dimension restart + 1)
            r.V = keep[1][:r.m + 1].T.copy()                # n x (m + 1)
            r.cycles = keep[5].value
            r.restart_x, r.restart_it = keep[3][:r.cycles].copy(), keep[4][:r.cycles].copy()
        return r

    def gmres(self, P, csc, b, x=None, restart=None, orth_meth="mgs", maxiter=None, abstol=0.0, reltol=RELTOL, probe=False):
        """the C loops of Identity / Jacobi / ILU0 / ILUAM; x = None: from zeros, else gmres! on a copy"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        return self._run(lambda *a: self.L.model_gmres(P.kind, n, _p(cp), _p(rv), _p(nz), _p(P.diag), _p(P.idiag), _p(P.fval), *a),
                         n, b, x, restart, orth_meth, maxiter, abstol, reltol, probe)

    def gmres_cb(self, M, n, b, x=None, restart=None, orth_meth="mgs", maxiter=None, abstol=0.0, reltol=RELTOL, probe=False):
        """the same loop with M.mul(v) and M.ldiv(v) behind the two function pointers"""
        def wrap(fn):
            def cb(_ctx, v, out):
                np.ctypeslib.as_array(out, (n,))[:] = fn(np.ctypeslib.as_array(v, (n,)).copy())
            return APPLY(cb)
        mul, ldiv = wrap(M.mul), wrap(M.ldiv)
        return self._run(lambda *a: self.L.model_gmres_cb(n, mul, ldiv, *a), n, b, x, restart, orth_meth, maxiter, abstol, reltol,
                         probe)
