"""ctypes binding of tests/matops_model.c (test infrastructure): SparseArrays' A*B, A+B / A-B and Diagonal scaling restated as
literal loops.  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "matops_model.c")
OP_ADD, OP_SUB = 0, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _csc(csc):
    cp, rv, nz = csc
    return np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64), np.ascontiguousarray(nz, np.float64)


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "matops_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC])
        L = C.CDLL(so)
        i64, vp, i32 = C.c_int64, C.c_void_p, C.c_int32
        L.model_matmul.argtypes = [i64, i64] + [vp] * 9
        L.model_matmul.restype = i64
        L.model_add.argtypes = [i64, i32] + [vp] * 9
        L.model_add.restype = i64
        L.model_diag_scale.argtypes = [i32, i64, vp, vp, vp, vp, vp]
        self.L = L

    def matmul(self, m, A, B):
        """A (m x k) * B (k x n) -> (colptr, rowval, nzval)"""
        ca, ra, za = _csc(A)
        cb, rb, zb = _csc(B)
        n = len(cb) - 1
        lens = np.diff(ca)
        cap = int(lens[rb - 1].sum()) if len(rb) else 0
        cp = np.empty(n + 1, np.int64)
        rv = np.empty(max(cap, 1), np.int64)
        nz = np.empty(max(cap, 1), np.float64)
        z = self.L.model_matmul(m, n, _p(ca), _p(ra), _p(za), _p(cb), _p(rb), _p(zb), _p(cp), _p(rv), _p(nz))
        return cp, rv[:z].copy(), nz[:z].copy()

    def add(self, A, B, op=OP_ADD):
        ca, ra, za = _csc(A)
        cb, rb, zb = _csc(B)
        n = len(ca) - 1
        cap = len(ra) + len(rb)
        cp = np.empty(n + 1, np.int64)
        rv = np.empty(max(cap, 1), np.int64)
        nz = np.empty(max(cap, 1), np.float64)
        z = self.L.model_add(n, op, _p(ca), _p(ra), _p(za), _p(cb), _p(rb), _p(zb), _p(cp), _p(rv), _p(nz))
        return cp, rv[:z].copy(), nz[:z].copy()

    def diag_scale(self, A, d, side):
        ca, ra, za = _csc(A)
        d = np.ascontiguousarray(d, np.float64)
        out = np.empty(max(len(za), 1), np.float64)
        self.L.model_diag_scale(side, len(ca) - 1, _p(ca), _p(ra), _p(za), _p(d), _p(out))
        return ca.copy(), ra.copy(), out[:len(za)].copy()
