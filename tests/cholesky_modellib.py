"""ctypes binding of tests/cholesky_model.c (test infrastructure): CholeskyFactorization's rule as plain loops.  The
ordering, the tree and the pattern are lu_modellib's: column j of L is the part of column j of the filled matrix B from the diagonal
on.  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses."""
import ctypes as C
import os
import subprocess

import numpy as np

import lu_modellib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cholesky_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class NotPosDef(Exception):
    """.position: the smallest position in c whose pivot fails (0-based), .column: A's column c[position] (0-based)"""

    def __init__(self, position, column):
        Exception.__init__(self, "position %d (column %d of A)" % (position, column))
        self.position, self.column = int(position), int(column)


class Model:
    def __init__(self, outdir, lu=None):
        so = os.path.join(str(outdir), "cholesky_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_chol_load.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_chol_load.restype = None
        L.model_chol_factor.argtypes = [i64, vp, vp, vp]
        L.model_chol_factor.restype = i64
        L.model_chol_solve.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        L.model_chol_solve.restype = None
        self.L = L
        self.lu = lu if lu is not None else lu_modellib.Model(outdir)

    def cholesky(self, csc, leaf_size=32, max_depth=48):
        return CholFact(self, csc, leaf_size, max_depth)


def with_diagonal(csc):
    """the pattern of csc with every diagonal position stored (values: zeros where added).  Self loops take no part in the graph:
    the ordering and struct are those of csc"""
    import scipy.sparse as sp
    cp, rv, nz = csc
    n = len(cp) - 1
    P = sp.csc_matrix((np.ones(len(rv)), np.asarray(rv) - 1, np.asarray(cp) - 1), shape=(n, n)) + sp.identity(n, format="csc")
    P = sp.csc_matrix(P)
    P.sort_indices()
    return P.indptr.astype(np.int64) + 1, P.indices.astype(np.int64) + 1, np.zeros(P.nnz)


class CholFact:
    """the model's factorization with its update state: .c (0-based), .level, .node_root, .nstart, .nsize, .L = (colptr, rowval,
    nzval) in Julia layout and positions of c, .stats; update(csc) is update!; ldiv / solve is u[c] = L' \\ (L \\ v[c]); .csc / .n:
    what the solver models read.  A failing pivot raises NotPosDef and leaves .failed set until an update succeeds."""

    def __init__(self, model, csc, leaf_size=32, max_depth=48):
        self.m, self.leaf_size, self.max_depth = model, int(leaf_size), int(max_depth)
        self.builds = 0
        self.failed = False
        self._construct(lu_modellib._csc(csc))

    def _construct(self, csc):
        cp, rv, nz = csc
        n = len(cp) - 1
        lu = self.m.lu
        c, level, root, nstart, nsize, anc, rounds, nodes = lu.nested_dissection(csc, self.leaf_size, self.max_depth)
        dcp, drv, dnz = with_diagonal(csc)
        bcp = np.empty(n + 1, np.int64)
        args = (n, _p(dcp), _p(drv), _p(dnz), rounds, _p(level), _p(anc), _p(c), _p(nstart), _p(nsize), _p(bcp))
        nnzb = lu.L.model_lu_fill(*args, None, None)
        assert nnzb >= 0
        brv, bnz = np.empty(nnzb, np.int64), np.empty(nnzb, np.float64)
        assert lu.L.model_lu_fill(*args, _p(brv), _p(bnz)) == nnzb
        col = np.repeat(np.arange(n, dtype=np.int64), np.diff(bcp))
        keep = brv - 1 >= col
        lrv = np.ascontiguousarray(brv[keep])
        lcp = np.ones(n + 1, np.int64)
        lcp[1:] += np.cumsum(np.bincount(col[keep], minlength=n)) if n else 0
        self.csc, self.n = csc, n
        self.c, self.level, self.node_root, self.nstart, self.nsize = c, level, root, nstart, nsize
        self.lcp, self.lrv = lcp, lrv
        self.stats = {"nnz": int(len(lrv)), "rounds": rounds, "deepest": int(level.max()) if n else 0, "nodes": nodes,
                      "largest_node": int(nsize.max()) if n else 0}
        self.builds += 1
        self._factor()

    def _factor(self):
        cp, rv, nz = self.csc
        lnz = np.zeros(len(self.lrv))
        self.failed = True
        if self.n:
            self.m.L.model_chol_load(self.n, _p(cp), _p(rv), _p(nz), _p(self.c), _p(self.lcp), _p(self.lrv), _p(lnz))
            bad = self.m.L.model_chol_factor(self.n, _p(self.lcp), _p(self.lrv), _p(lnz))
            if bad:
                raise NotPosDef(bad - 1, self.c[bad - 1])
        self.failed = False
        self.L = (self.lcp, self.lrv, lnz)

    def update(self, csc):
        csc = lu_modellib._csc(csc)
        if not (np.array_equal(csc[0], self.csc[0]) and np.array_equal(csc[1], self.csc[1])):
            self._construct(csc)
            return self
        self.csc = csc  # the values only: the load and the factor on the kept ordering and pattern
        self._factor()
        return self

    def ldiv(self, v, inplace=False):
        assert not self.failed
        v = np.asarray(v, np.float64)
        if self.n == 0:
            return v if inplace else v.copy()
        y = np.ascontiguousarray(v[self.c])
        self.m.L.model_chol_solve(self.n, _p(self.lcp), _p(self.lrv), _p(self.L[2]), _p(self.nstart), _p(self.nsize), _p(y))
        out = v if inplace else np.empty_like(v)
        out[self.c] = y
        return out

    solve = ldiv

    def dense_L(self):
        Lm = np.zeros((self.n, self.n))
        for j in range(self.n):
            q = slice(self.lcp[j] - 1, self.lcp[j + 1] - 1)
            Lm[self.lrv[q] - 1, j] = self.L[2][q]
        return Lm


def symmetric_dense(csc):
    """Symmetric(A): the stored upper triangle mirrored"""
    A = lu_modellib.dense_of(csc)
    U = np.triu(A)
    return U + np.triu(A, 1).T


def dense_cholesky_position(S):
    """the first column whose pivot fails in a dense sequential Cholesky of S, or -1"""
    F = np.array(S, np.float64)
    n = len(F)
    for j in range(n):
        if not F[j, j] > 0:
            return j
        F[j, j] = np.sqrt(F[j, j])
        F[j + 1:, j] /= F[j, j]
        F[j + 1:, j + 1:] -= np.outer(F[j + 1:, j], F[j + 1:, j])
    return -1
