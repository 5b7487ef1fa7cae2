"""ctypes binding of tests/lu_model.c (test infrastructure): LUFactorization's nested-dissection ordering, its tree and the filled,
reordered matrix B; the numerics are iluam_modellib's factorization and ldiv! over B with v[c], scattered back.  Beside it a dense
NumPy elimination without pivoting, which tests/test_lu_model.py holds the predicted pattern to.  Built with
gcc -O1 -ffp-contract=off into a directory the caller chooses."""
import ctypes as C
import os
import subprocess

import numpy as np

import iluam_modellib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lu_model.c")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Model:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "lu_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        i64, vp = C.c_int64, C.c_void_p
        L.model_lu_dissect.argtypes = [i64, vp, vp, i64, i64, vp, vp]
        L.model_lu_dissect.restype = i64
        L.model_lu_perm.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp]
        L.model_lu_perm.restype = i64
        L.model_lu_fill.argtypes = [i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.model_lu_fill.restype = i64
        self.L = L
        self.iluam = iluam_modellib.Model(outdir)

    def lu(self, csc, leaf_size=32, max_depth=48):
        return LuFact(self, csc, leaf_size, max_depth)

    def nested_dissection(self, csc, leaf_size=32, max_depth=48):
        """-> (c, level, node_root, nstart, nsize, anc, rounds, nodes), everything 0-based"""
        cp, rv = (np.ascontiguousarray(a, np.int64) for a in csc[:2])
        n = len(cp) - 1
        level, anc = np.empty(max(n, 1), np.int64), np.empty(max((max_depth + 1) * n, 1), np.int64)
        rounds = self.L.model_lu_dissect(n, _p(cp), _p(rv), leaf_size, max_depth, _p(level), _p(anc))
        c, root, nstart, nsize = (np.empty(max(n, 1), np.int64) for _ in range(4))
        nodes = self.L.model_lu_perm(n, rounds, _p(level), _p(anc), _p(c), _p(root), _p(nstart), _p(nsize))
        return c[:n], level[:n], root[:n], nstart[:n], nsize[:n], anc, int(rounds), int(nodes)


def _csc(csc):
    return tuple(np.array(a, dtype=t, copy=True) for a, t in zip(csc, (np.int64, np.int64, np.float64)))


class LuFact:
    """the model's factorization with its update state: .c (0-based), .level, .node_root, .B = (colptr, rowval, nzval), .fval, .diag,
    .stats; update(csc) is update! for A's new arrays; ldiv / solve is u[c] = ILUAM(B) \\ v[c]; .csc / .n: what the solver models read"""

    def __init__(self, model, csc, leaf_size=32, max_depth=48):
        self.m, self.leaf_size, self.max_depth = model, int(leaf_size), int(max_depth)
        self.builds = 0
        self._construct(_csc(csc))

    def _construct(self, csc):
        cp, rv, nz = csc
        n = len(cp) - 1
        c, level, root, nstart, nsize, anc, rounds, nodes = self.m.nested_dissection(csc, self.leaf_size, self.max_depth)
        bcp = np.empty(n + 1, np.int64)
        args = (n, _p(cp), _p(rv), _p(nz), rounds, _p(level), _p(anc), _p(c), _p(nstart), _p(nsize), _p(bcp))
        nnzb = self.m.L.model_lu_fill(*args, None, None)
        if nnzb < 0:
            raise ValueError("column %d of B (column %d of A) has no stored diagonal" % (-nnzb, c[-nnzb - 1] + 1))
        brv, bnz = np.empty(nnzb, np.int64), np.empty(nnzb, np.float64)
        assert self.m.L.model_lu_fill(*args, _p(brv), _p(bnz)) == nnzb
        self.csc, self.n = csc, n
        self.c, self.level, self.node_root, self.nstart, self.nsize = c, level, root, nstart, nsize
        self.B = (bcp, brv, bnz)
        self.stats = {"nnz": int(nnzb), "rounds": rounds, "deepest": int(level.max()) if n else 0, "nodes": nodes,
                      "largest_node": int(nsize.max()) if n else 0}
        self.builds += 1
        self._factor()

    def _factor(self):
        if self.n:
            self.fval, self.diag = self.m.iluam.factor(self.B)
        else:
            self.fval, self.diag = np.empty(0), np.empty(0, np.int64)

    def update(self, csc):
        csc = _csc(csc)
        if not (np.array_equal(csc[0], self.csc[0]) and np.array_equal(csc[1], self.csc[1])):
            self._construct(csc)
            return self
        # the values only: one gather through the positions B's entries came from
        A = dense_positions(csc)
        bcp, brv, bnz = self.B
        for l in range(self.n):
            for q in range(bcp[l] - 1, bcp[l + 1] - 1):
                at = A.get((self.c[brv[q] - 1], self.c[l]))
                bnz[q] = 0.0 if at is None else csc[2][at]
        self.csc = csc
        self._factor()
        return self

    def ldiv(self, v, inplace=False):
        v = np.asarray(v, np.float64)
        if self.n == 0:
            return v if inplace else v.copy()
        x = self.m.iluam.ldiv(self.B, self.fval, self.diag, v[self.c])
        out = v if inplace else np.empty_like(v)
        out[self.c] = x
        return out

    solve = ldiv


def dense_positions(csc):
    """{(row, column) 0-based: position in nzval}"""
    cp, rv, _ = csc
    return {(int(rv[q] - 1), j): q for j in range(len(cp) - 1) for q in range(cp[j] - 1, cp[j + 1] - 1)}


def dense_of(csc):
    cp, rv, nz = csc
    n = len(cp) - 1
    A = np.zeros((n, n))
    for j in range(n):
        A[np.asarray(rv[cp[j] - 1:cp[j + 1] - 1]) - 1, j] = nz[cp[j] - 1:cp[j + 1] - 1]
    return A


def pattern_of(cp, rv):
    n = len(cp) - 1
    P = np.zeros((n, n), bool)
    for j in range(n):
        P[np.asarray(rv[cp[j] - 1:cp[j + 1] - 1]) - 1, j] = True
    return P


def dense_lu_nopivot(A):
    """L\\U of a dense elimination without pivoting, in place of a copy"""
    F = np.array(A, np.float64)
    n = len(F)
    for k in range(n):
        F[k + 1:, k] /= F[k, k]
        F[k + 1:, k + 1:] -= np.outer(F[k + 1:, k], F[k, k + 1:])
    return F


# ---- the small matrices both test files use (scipy CSC, a full diagonal unless said otherwise) -----------------------------------
def csc_of(S):
    import scipy.sparse as sp
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.astype(np.float64)


def dominant(P, seed=3):
    """seeded values on the boolean pattern P (diagonal added), made strictly diagonally dominant by rows and columns: no
    cancellation hides an entry of the elimination"""
    import scipy.sparse as sp
    n = len(P)
    rng = np.random.default_rng(seed)
    M = np.where(P, rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)), 0.0)
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    keep = P | np.eye(n, dtype=bool)
    return sp.csc_matrix(np.where(keep, M, 0.0))      # (every kept value is non-zero: the stored pattern is `keep`)


def edges_pattern(n, edges, symmetric=True):
    P = np.zeros((n, n), bool)
    for i, j in edges:
        P[i, j] = True
        if symmetric:
            P[j, i] = True
    return P


def path(n):
    return dominant(edges_pattern(n, [(i, i + 1) for i in range(n - 1)]))


def arrow(n):
    return dominant(edges_pattern(n, [(0, i) for i in range(1, n)]))


def star(entries):
    """a hub (vertex 0) whose column holds `entries` stored rows, the diagonal among them; the spokes are stored one way only, in
    the hub's column: the hub's row holds its diagonal alone"""
    return dominant(edges_pattern(entries, [(i, 0) for i in range(1, entries)], symmetric=False))


def clique(n):
    return dominant(np.ones((n, n), bool))


def two_cliques(m):
    P = np.zeros((2 * m, 2 * m), bool)
    P[:m, :m] = P[m:, m:] = True
    P[m - 1, m] = P[m, m - 1] = True
    return dominant(P)


def grid_edges(nx, ny, base=0):
    e = []
    for y in range(ny):
        for x in range(nx):
            v = base + y * nx + x
            if x + 1 < nx:
                e.append((v, v + 1))
            if y + 1 < ny:
                e.append((v, v + nx))
    return e


def components_of(sizes):
    """paths of the given sizes side by side"""
    e, base = [], 0
    for m in sizes:
        e += [(base + i, base + i + 1) for i in range(m - 1)]
        base += m
    return dominant(edges_pattern(base, e))


def block_diagonal():
    """six 7 x 5 grids and five 3-paths"""
    e, base = [], 0
    for _ in range(6):
        e += grid_edges(7, 5, base)
        base += 35
    for _ in range(5):
        e += [(base, base + 1), (base + 1, base + 2)]
        base += 3
    return dominant(edges_pattern(base, e))


def random_pattern(n, symmetric, density, seed):
    rng = np.random.default_rng(seed)
    P = rng.random((n, n)) < density
    if symmetric:
        P = P | P.T
    return dominant(P, seed)
