"""ctypes binding of tests/iluk_model.c (test infrastructure): the filled matrix B of ILUKPreconditioner by the sequential
level-of-fill rule, literally; the numeric side is iluam_modellib's Model applied to B.  Beside it, in plain Python: the parallel form
of the rule the device uses (one bounded breadth-first search per column) and an exhaustive fill-path enumeration, which
tests/test_iluk_model.py holds to the sequential rule.  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses."""
import ctypes as C
import os
import subprocess

import numpy as np

import iluam_modellib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "iluk_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "iluk_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_iluk.argtypes = [i64, vp, vp, vp, i64, vp, vp, vp, vp, i64]
        L.model_iluk.restype = i64
        self.L = L
        self.iluam = iluam_modellib.Model(outdir)

    def fill(self, csc, K):
        """B of the Julia CSC arrays csc for the level K -> ((colptr, rowval, nzval), int32 level of every stored entry)"""
        cp, rv, nz = (np.ascontiguousarray(cp_, t) for cp_, t in zip(csc, (np.int64, np.int64, np.float64)))
        n = len(cp) - 1
        bcp = np.empty(n + 1, np.int64)
        nnzb = self.L.model_iluk(n, _p(cp), _p(rv), _p(nz), int(K), _p(bcp), None, None, None, -1)
        assert nnzb >= 0
        brv, bnz, blev = np.empty(nnzb, np.int64), np.empty(nnzb, np.float64), np.empty(nnzb, np.int32)
        assert self.L.model_iluk(n, _p(cp), _p(rv), _p(nz), int(K), _p(bcp), _p(brv), _p(bnz), _p(blev), nnzb) == nnzb
        return (bcp, brv, bnz), blev

    def precon(self, csc, K):
        """ILUKPreconditioner(A, K) -> IlukPrecon: B, its levels and iluAM(B).  A column of A without a stored diagonal is refused,
        as iluAM(A) refuses it (the literal rule would fill such a diagonal position from lev(j,k) and lev(k,j); the preconditioner
        is defined for matrices that store every diagonal entry, where the diagonal has level 0)"""
        cp, rv = np.asarray(csc[0]), np.asarray(csc[1])
        for j in range(len(cp) - 1):
            if j + 1 not in rv[cp[j] - 1:cp[j + 1] - 1]:
                raise ValueError("column %d has no stored diagonal" % (j + 1))
        B, lev = self.fill(csc, K)
        fval, diag = self.iluam.factor(B)
        return IlukPrecon(self, csc, B, lev, fval, diag)


class IlukPrecon:
    """the model's preconditioner: .B, .lev, .fval, .diag, ldiv, and mul with the matrix A it was made from -- the object the
    statement-by-statement solver models (.mul / .ldiv) are driven with"""

    def __init__(self, model, csc, B, lev, fval, diag):
        self.m, self.B, self.lev, self.fval, self.diag = model, B, lev, fval, diag
        self.csc = tuple(np.array(a, copy=True) for a in csc)
        self.n = len(self.csc[0]) - 1

    def ldiv(self, v, inplace=False):
        return self.m.iluam.ldiv(self.B, self.fval, self.diag, v, inplace=inplace)


def columns_of(cp, rv):
    """the stored rows (0-based) of every column of the Julia arrays (colptr, rowval)"""
    return [[int(r) - 1 for r in rv[cp[j] - 1:cp[j + 1] - 1]] for j in range(len(cp) - 1)]


def transpose_columns(cols):
    out = [[] for _ in cols]
    for j, col in enumerate(cols):
        for i in col:
            out[i].append(j)
    return out


def search(adj, j, K):
    """The bounded, level-synchronous breadth-first search from column j: the neighbours of a vertex u are adj[u], dist(j) = 0.
    A first-visited w > j is emitted with the level dist(u) and never expanded; a first-visited w < j is enqueued with dist(u) + 1
    while that is <= K.  -> ({w: level}, size of the visited set as the device counts it: j, every enqueued vertex and every
    vertex emitted beyond level 0 -- the level-0 rows are column j itself and need no table)"""
    visited = {j}
    emitted = {}
    frontier, d = [j], 0
    while frontier:
        nxt = []
        for u in frontier:
            for w in adj[u]:
                if w in visited:
                    continue
                if w > j:
                    visited.add(w)
                    emitted[w] = d
                elif d + 1 <= K:
                    visited.add(w)
                    nxt.append(w)
        frontier, d = nxt, d + 1
    return emitted, len(visited) - sum(1 for l in emitted.values() if l == 0)


def parallel_levels(cp, rv, K):
    """The parallel form of the rule -> ({(i, j): level} of every stored position of B, visited-set sizes of the lower searches,
    ... of the upper searches).  Column j of B below the diagonal is search(A's columns, j); the same search over transpose(A)
    gives row j to the right of the diagonal: an emitted (w, j) there is the entry (j, w); the diagonal is A's."""
    cols = columns_of(cp, rv)
    tcols = transpose_columns(cols)
    n = len(cols)
    lev, vl, vu = {}, [], []
    for j in range(n):
        if j in cols[j]:
            lev[(j, j)] = 0
        em, nv = search(cols, j, K)
        vl.append(nv)
        for w, l in em.items():
            assert (w, j) not in lev
            lev[(w, j)] = l
        em, nv = search(tcols, j, K)
        vu.append(nv)
        for w, l in em.items():
            assert (j, w) not in lev
            lev[(j, w)] = l
    return lev, vl, vu


def fill_path_levels(cp, rv, K):
    """lev(i,j) + 1 = the length of the shortest path i -> j in the graph of A (an edge i -> j where A stores (i,j)) whose interior
    vertices are all < min(i,j), by exhaustive enumeration of the simple paths (n <= 10) -> {(i, j): level} for level <= K"""
    cols = columns_of(cp, rv)
    n = len(cols)
    succ = transpose_columns(cols)          # succ[i] = the columns j with a stored (i, j)
    best = {}

    def walk(i, at, seen, length):
        for j in succ[at]:
            if j in seen:
                continue
            key = (i, j)
            if length + 1 < best.get(key, 1 << 60):
                best[key] = length + 1
            # j may become an interior vertex of a path i -> t only if j < min(i, t)
            if j < i:
                walk_interior(i, j, seen | {j}, length + 1, j)

    def walk_interior(i, at, seen, length, top):
        """paths from i whose interior so far has the largest vertex `top`: an end t needs top < min(i, t)"""
        for j in succ[at]:
            if j in seen:
                continue
            if j > top:                      # a legal end of the path
                key = (i, j)
                if length + 1 < best.get(key, 1 << 60):
                    best[key] = length + 1
            if j < i:                        # ... and a legal interior vertex of a longer one
                walk_interior(i, j, seen | {j}, length + 1, max(top, j))

    for i in range(n):
        walk(i, i, {i}, 0)
    for i in range(n):                       # the diagonal is a position like any other: stored or not
        best.pop((i, i), None)
        if i in cols[i]:
            best[(i, i)] = 1
    return {key: l - 1 for key, l in best.items() if l - 1 <= K}


def levels_as_dict(B, lev):
    cp, rv, _ = B
    out = {}
    for j in range(len(cp) - 1):
        for q in range(cp[j] - 1, cp[j + 1] - 1):
            out[(int(rv[q]) - 1, j)] = int(lev[q])
    return out
