"""ctypes binding of tests/bicgstabl_model.c (test infrastructure): BiCGStab(l) as esp_bicgstabl states it, as literal loops.
bicgstabl_model.c includes cg_model.c (ldiv!, mul! and the ordered dot product are its), so this Model offers everything
cg_modellib's does (precon, mul, ldiv, dot) plus bicgstabl.  Built with gcc -O1 -ffp-contract=off into a directory the caller
chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

import cg_modellib
from cg_modellib import KINDS, RELTOL, Precon, _p  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bicgstabl_model.c")


def history_len(max_mv_products, l):
    return -(-max_mv_products // (2 * l)) + 1


class Model(cg_modellib.Model):
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "bicgstabl_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        L.model_cg_dot.argtypes = [i64, vp, vp]
        L.model_cg_dot.restype = f64
        L.model_bicgstabl.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i64, f64, f64, vp, C.POINTER(i64),
                                      C.POINTER(i32)]
        L.model_bicgstabl.restype = i64
        L.model_bicgstabl_gamma.argtypes = [i32, vp, vp]
        L.model_bicgstabl_gamma.restype = None
        L.model_jacobi_ldiv.argtypes = [i64, vp, vp, vp]
        L.model_ilu0_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_iluam_ldiv.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_mul.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_diag.argtypes = [i64, vp, vp, vp]
        L.model_iluam_diag.restype = i64
        L.model_iluam_factor.argtypes = [i64, vp, vp, vp, vp, vp]
        L.model_iluam_factor.restype = None
        self.L = L

    def gamma(self, M):
        """gamma[1..l] of the (l+1) x (l+1) Gram matrix M"""
        l = len(M) - 1
        full = np.zeros((5, 5))
        full[:l + 1, :l + 1] = M
        g = np.zeros(l + 1)
        self.L.model_bicgstabl_gamma(l, _p(full), _p(g))
        return g[1:].copy()

    def bicgstabl(self, P, csc, b, l=2, x=None, max_mv_products=None, abstol=0.0, reltol=RELTOL, r_shadow=None):
        """-> (x, history (iterations + 1 norms), outer iterations, matrix-vector products, converged); x = None: from zeros,
        else bicgstabl! on a copy"""
        cp, rv, nz = self._csc(csc)
        n = len(cp) - 1
        b = np.ascontiguousarray(b, np.float64)
        zero = 1 if x is None else 0
        x = np.zeros(n) if x is None else np.array(x, np.float64)
        max_mv_products = n if max_mv_products is None else max_mv_products
        rsh = None if r_shadow is None else np.ascontiguousarray(r_shadow, np.float64)
        hist = np.empty(history_len(max_mv_products, l))
        conv, mv = C.c_int32(), C.c_int64()
        it = self.L.model_bicgstabl(P.kind, n, _p(cp), _p(rv), _p(nz), _p(P.diag), _p(P.idiag), _p(P.fval), l, _p(b), _p(x), _p(rsh),
                                    zero, max_mv_products, abstol, reltol, _p(hist), C.byref(mv), C.byref(conv))
        assert it >= 0
        return x, hist[:it + 1].copy(), it, mv.value, bool(conv.value)


def convdiff_triplets(nx, ny, nz, pe, seed=1):
    """the upwind convection-diffusion matrix as unique 1-based triplets (I, J, V), x running fastest:
    A = I (x) I (x) (L + pe C) + I (x) (L + pe/2 C) (x) I + L (x) I (x) I (the last term for nz > 1 only), L = tridiag(-1, 2, -1),
    C = bidiag(sub -1, diag 1); every stored value scaled by 1 + 0.1 u, u uniform in [0, 1) from a seeded generator"""
    import scipy.sparse as sp

    def L(m):
        return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")

    def Cm(m):
        return sp.diags([-np.ones(m - 1), np.ones(m)], [-1, 0], format="csr")

    ex, ey, ez = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    S = sp.kron(ez, sp.kron(ey, L(nx) + pe * Cm(nx))) + sp.kron(ez, sp.kron(L(ny) + 0.5 * pe * Cm(ny), ex))
    if nz > 1:
        S = S + sp.kron(L(nz), sp.kron(ey, ex))
    S = sp.coo_matrix(S)
    S.sum_duplicates()
    V = S.data * (1.0 + 0.1 * np.random.default_rng(seed).random(len(S.data)))
    return S.row.astype(np.int64) + 1, S.col.astype(np.int64) + 1, V


def csc_arrays(n, I, J, V):
    """Julia's CSC arrays (1-based colptr and rowval, nzval) of unique triplets"""
    import scipy.sparse as sp
    S = sp.csc_matrix((V, (I - 1, J - 1)), shape=(n, n))
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)
