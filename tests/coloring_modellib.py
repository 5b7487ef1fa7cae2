"""ctypes binding of tests/coloring_model.c (test infrastructure): the multicolour ordering of include/esparse_hip.h
(esp_graph_coloring, esp_precon_colored_create) as literal loops -- the rounds, the permutation, A[c,c] -- plus a plain-Python
restatement of the rule over sets, and the model of the preconditioner: block_precon_modellib's BlockModel over the single partition c,
which is precon_model.c / iluam_model.c applied to A[c,c] with v[c] and scattered back, with the solver loops around it.  Built with
gcc -O1 -ffp-contract=off into a directory the caller chooses (a pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "coloring_model.c")
AMG_LONG = 32        # csrc/amg.hpp: a vertex with a longer column or row is folded by its whole wave


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Coloring:
    """ncolors, color (0-based, per vertex), c (0-based, the vertices by (colour, index)), ptr (ncolors + 1 offsets into c)"""

    def __init__(self, ncolors, color, c, ptr):
        self.ncolors, self.color, self.c, self.ptr = ncolors, color, c, ptr

    def lists(self):
        """the reference's `coloring`: a list of 1-based index arrays"""
        return [self.c[a:b] + 1 for a, b in zip(self.ptr[:-1], self.ptr[1:])]


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "coloring_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_coloring.argtypes = [i64, vp, vp, vp]
        L.model_coloring.restype = i64
        L.model_color_perm.argtypes = [i64, i64, vp, vp, vp]
        L.model_color_perm.restype = None
        L.model_reorder.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        L.model_reorder.restype = None
        self.L = L

    def coloring(self, cp, rv):
        cp, rv = np.ascontiguousarray(cp, np.int64), np.ascontiguousarray(rv, np.int64)
        n = len(cp) - 1
        color = np.empty(max(n, 1), np.int64)
        nc = self.L.model_coloring(n, _p(cp), _p(rv), _p(color))
        c, ptr = np.empty(max(n, 1), np.int64), np.empty(nc + 1, np.int64)
        self.L.model_color_perm(n, nc, _p(color), _p(c), _p(ptr))
        return Coloring(int(nc), color[:n], c[:n], ptr)

    def reorder(self, csc, c):
        """A[c,c] as Julia CSC arrays"""
        cp, rv, nz = (np.ascontiguousarray(a, t) for a, t in zip(csc, (np.int64, np.int64, np.float64)))
        n = len(cp) - 1
        c = np.ascontiguousarray(c, np.int64)
        bcp, brv, bnz = np.empty(n + 1, np.int64), np.empty(max(len(rv), 1), np.int64), np.empty(max(len(rv), 1), np.float64)
        self.L.model_reorder(n, _p(cp), _p(rv), _p(nz), _p(c), _p(bcp), _p(brv), _p(bnz))
        return bcp, brv[:len(rv)], bnz[:len(rv)]


def mix(i):
    """the 32-bit mixer of the fixed hash (csrc/amg.hpp), applied to i + 1"""
    m = 0xFFFFFFFF
    x = (i + 1) & m
    x ^= x >> 16
    x = (x * 0x7feb352d) & m
    x ^= x >> 15
    x = (x * 0x846ca68b) & m
    x ^= x >> 16
    return x


def key(i):
    return (mix(i) << 32) | i


def neighbours(cp, rv):
    """the neighbour sets of the rule: j in N(i) iff i != j and (i,j) or (j,i) is stored"""
    n = len(cp) - 1
    N = [set() for _ in range(n)]
    for j in range(n):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            i = int(rv[k]) - 1
            if i != j:
                N[i].add(j)
                N[j].add(i)
    return N


def python_coloring(cp, rv):
    """the rule of include/esparse_hip.h over sets: -> (ncolors, colour of every vertex)"""
    n = len(cp) - 1
    N = neighbours(cp, rv)
    color = [-1] * n
    U = set(range(n))
    r = 0
    while U:
        chosen = [i for i in U if all(key(i) > key(j) for j in N[i] if j in U)]
        for i in chosen:
            color[i] = r
        U -= set(chosen)
        r += 1
    return r, np.array(color, np.int64)


def dominant_nonsymmetric(n, seed):
    """a seeded strictly diagonally dominant (by columns and by rows) non-symmetric matrix as Julia CSC arrays: the generator of the
    ILU(k) tests (tests/test_iluk_model.py), restated"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    M = np.where(rng.random((n, n)) < 0.08, rng.standard_normal((n, n)), 0.0)
    np.fill_diagonal(M, 0.0)
    M[np.arange(1, n), np.arange(n - 1)] = -1.0     # irreducible
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    S = sp.csc_matrix(M)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def replay_pair(gm, bm, orc, csc, col):
    """the model pair of the replay of the reference's test/test_parilu0.jl: b = A*ones;
    gmres(A, b, Pl = ParallelILU0Preconditioner(A)) in A's numbering, and gmres(A_r, b_r, Pl = ILU0Preconditioner(A_r)) on
    A_r, b_r = reorderlinsys(A, b, coloring).  gm: gmres_modellib.Model, bm: block_precon_modellib.Model, col: a Coloring.
    -> (the two Results, b)"""
    n = len(csc[0]) - 1
    b = bm.mul(csc, np.ones(n))
    par = gm.gmres_cb(colored_model(bm, orc, "ilu0", csc, col.c), n, b)
    Ar = reorder_py(csc, col.c)
    ser = gm.gmres(gm.precon("ilu0", Ar, orc), Ar, np.ascontiguousarray(b[col.c]))
    return par, ser, b


def reorder_py(csc, c):
    """A[c,c] with NumPy (the check of model_reorder, and reorderlinsys' model)"""
    cp, rv, nz = csc
    n = len(cp) - 1
    new = np.empty(n, np.int64)
    new[np.asarray(c)] = np.arange(n)
    bcp, brv, bnz = [1], [], []
    for j in c:
        ks = list(range(cp[j] - 1, cp[j + 1] - 1))
        ks.sort(key=lambda k: new[rv[k] - 1])
        brv.extend(new[rv[k] - 1] + 1 for k in ks)
        bnz.extend(nz[k] for k in ks)
        bcp.append(bcp[-1] + len(ks))
    return np.array(bcp, np.int64), np.array(brv, np.int64), np.array(bnz, np.float64)


def colored_model(block_model, orc, kind, csc, c):
    """the preconditioner's model: u[c] = kind(A[c,c]) \\ v[c] -- BlockModel over the one partition c (0-based), with its cg,
    bicgstabl and simple loops; .factor(True) is the ILUAM factor in the position order of A[c,c]"""
    from block_precon_modellib import BlockModel
    return BlockModel(block_model, orc, kind, csc, [np.asarray(c, np.int64)])
