"""ctypes binding of tests/linalg_model.c (test infrastructure): SparseArrays' transpose, transpose(A)*x, issymmetric and the
general-branch opnorm loops restated as literal loops; plus the norms of a value vector as SparseArrays / LinearAlgebra define them
(exact where the reference is, math.fsum-based references where it calls BLAS).  Built with gcc -O1 -ffp-contract=off into a
directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "linalg_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _csc(csc):
    cp, rv, nz = csc
    return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "linalg_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_transpose.argtypes = [i64, i64] + [vp] * 6
        L.model_mul_transpose.argtypes = [i64] + [vp] * 5
        L.model_opnorm1.argtypes = [i64, vp, vp]
        L.model_opnorm1.restype = C.c_double
        L.model_opnorminf.argtypes = [i64, i64, vp, vp, vp]
        L.model_opnorminf.restype = C.c_double
        L.model_issymmetric.argtypes = [i64, i64, vp, vp, vp]
        L.model_issymmetric.restype = C.c_int32
        self.L = L

    def transpose(self, m, A):
        """copy(transpose(A)) of an m x n CSC -> (colptr, rowval, nzval) of the n x m result"""
        cp, rv, nz = _csc(A)
        n = len(cp) - 1
        cpT = np.empty(m + 1, np.int64)
        rvT = np.empty(max(len(rv), 1), np.int64)
        nzT = np.empty(max(len(rv), 1), np.float64)
        self.L.model_transpose(m, n, _p(cp), _p(rv), _p(nz), _p(cpT), _p(rvT), _p(nzT))
        return cpT, rvT[:len(rv)].copy(), nzT[:len(rv)].copy()

    def mul_transpose(self, A, x):
        cp, rv, nz = _csc(A)
        n = len(cp) - 1
        x = np.ascontiguousarray(x, np.float64)
        r = np.empty(max(n, 1), np.float64)
        self.L.model_mul_transpose(n, _p(cp), _p(rv), _p(nz), _p(x), _p(r))
        return r[:n].copy()

    def opnorm_general(self, m, A, p):
        cp, rv, nz = _csc(A)
        n = len(cp) - 1
        if p == 1:
            return self.L.model_opnorm1(n, _p(cp), _p(nz))
        assert p == math.inf
        return self.L.model_opnorminf(m, n, _p(cp), _p(rv), _p(nz))

    def issymmetric(self, m, A):
        cp, rv, nz = _csc(A)
        return bool(self.L.model_issymmetric(m, len(cp) - 1, _p(cp), _p(rv), _p(nz)))


def norm_exact(v, p):
    """norm(v, p) of LinearAlgebra for the exact cases (p = Inf, -Inf, 0) -- bitwise, NaN propagating; None for the others"""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return 0.0
    a = np.abs(v)
    if p == math.inf:
        return math.nan if np.isnan(a).any() else float(a.max())
    if p == -math.inf:
        return math.nan if np.isnan(a).any() else float(a.min())
    if p == 0:
        return float(np.count_nonzero(~(v == 0.0)))  # (!iszero: a NaN counts)
    return None


def norm_ref(v, p):
    """norm(v, p) exactly rounded from the terms (math.fsum over scaled powers; the reference's BLAS / generic_normp results lie
    within 1e-13 of it): NaN gives NaN, Inf without NaN gives Inf"""
    e = norm_exact(v, p)
    if e is not None:
        return e
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    if np.isnan(a).any():
        return math.nan
    if p > 0 and np.isinf(a).any():
        return math.inf
    if p == 1:
        return math.fsum(a.tolist())
    s = float(a.max()) if p > 0 else float(a.min())
    if s == 0.0:  # (p < 0 with a zero among the values: |0|^p = Inf, Inf^(1/p) = 0)
        return 0.0
    terms = [(float(x) / s) ** p for x in a]
    return s * math.fsum(terms) ** (1.0 / p)
