"""Independent model of BlockPreconditioner (src/factorizations/blockpreconditioner.jl; test infrastructure): the reference's
own shape -- every A[part, part] extracted with plain NumPy loops, factorized and solved on its own with the existing models
(precon_model.c, iluam_model.c through cg_modellib's Model.precon / .ldiv), the results scattered back -- and the cg, bicgstabl
and simple! loops of include/esparse_hip.h restated with that ldiv and the models' own dot and mul.  Nothing here knows of the
device's single block matrix; block_matrix() restates what the header says B holds, for the tests that read B back."""
import ctypes as C

import numpy as np

import bicgstabl_modellib
from bicgstabl_modellib import RELTOL  # noqa: F401  (re-exported for the tests)


class Model(bicgstabl_modellib.Model):
    """bicgstabl_model.c's library (precon, ldiv, mul, dot, gamma, bicgstabl) with cg_model.c's model_cg declared as well"""

    def __init__(self, outdir):
        super().__init__(outdir)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        self.L.model_cg.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, f64, f64, vp, C.POINTER(i32)]
        self.L.model_cg.restype = i64


def check_partitioning(parts, n):
    """0-based index arrays that together hold every index 0..n-1 exactly once"""
    parts = [np.asarray(p, np.int64).reshape(-1) for p in parts]
    allidx = np.concatenate(parts) if parts else np.empty(0, np.int64)
    assert len(allidx) == n and np.array_equal(np.sort(allidx), np.arange(n))
    return parts


def increasing(parts):
    return all(np.all(np.diff(p) > 0) for p in parts)


def extract_block(csc, part):
    """A[part, part] as Julia CSC arrays (1-based), rows ascending in every column: plain loops"""
    cp, rv, nz = csc
    n = len(cp) - 1
    local = np.full(n, -1, np.int64)
    for k, i in enumerate(part):
        local[i] = k
    bcp, brv, bnz = [1], [], []
    for j in part:
        col = []
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            i = local[rv[k] - 1]
            if i >= 0:
                col.append((i + 1, k))
        col.sort()                                # (distinct rows)
        brv.extend(r for r, _ in col)
        bnz.extend(nz[k] for _, k in col)
        bcp.append(bcp[-1] + len(col))
    return np.array(bcp, np.int64), np.array(brv, np.int64), np.array(bnz, np.float64)


def block_matrix(csc, parts, permuted):
    """what include/esparse_hip.h says B holds: exactly the stored A[i,j] with part(i) == part(j), bits kept; in A's numbering
    (identity path) or renumbered by new(i), the position of i in the concatenation of the partitions (permuted path), rows
    ascending in every column"""
    cp, rv, nz = csc
    n = len(cp) - 1
    part_of, new = np.empty(n, np.int64), np.empty(n, np.int64)
    k = 0
    for ip, p in enumerate(parts):
        for i in p:
            part_of[i], new[i] = ip, k
            k += 1
    cols = [[] for _ in range(n)]
    for j in range(n):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            i = rv[k] - 1
            if part_of[i] == part_of[j]:
                cols[new[j] if permuted else j].append(((new[i] if permuted else i) + 1, k))
    bcp, brv, src = [1], [], []
    for col in cols:
        col.sort()
        brv.extend(r for r, _ in col)
        src.extend(k for _, k in col)
        bcp.append(bcp[-1] + len(col))
    src = np.array(src, np.int64)
    return np.array(bcp, np.int64), np.array(brv, np.int64), np.asarray(nz, np.float64)[src], src


class BlockModel:
    """the reference's BlockPreconditioner over host CSC arrays: update! at construction, ldiv, and the solvers with it"""

    def __init__(self, model, orc, kind, csc, parts):
        self.m, self.kind = model, kind
        self.csc = tuple(np.array(a, copy=True) for a in csc)   # (the solvers multiply with the matrix as it was handed in)
        self.n = len(self.csc[0]) - 1
        self.parts = check_partitioning(parts, self.n)
        self.blocks = [extract_block(self.csc, p) for p in self.parts]          # AP = A[part, part]
        self.facts = [model.precon(kind, b, orc) if len(p) else None for b, p in zip(self.blocks, self.parts)]   # FP = factorization(AP)

    def ldiv(self, v):
        """ldiv!(u, p, v): uu = facts[ipart] \\ v[part]; view(u, part) .= uu"""
        v = np.asarray(v, np.float64)
        u = np.empty(self.n)
        for p, b, f in zip(self.parts, self.blocks, self.facts):
            if len(p):
                u[p] = self.m.ldiv(f, b, np.ascontiguousarray(v[p]))
        return u

    def factor(self, permuted):
        """the ILUAM factors of all blocks in B's position order (see block_matrix)"""
        assert self.kind == "iluam"
        cp, rv, nz = self.csc
        out = np.empty(len(nz))
        for p, b, f in zip(self.parts, self.blocks, self.facts):
            if len(p) == 0:
                continue
            local = np.full(self.n, -1, np.int64)
            local[p] = np.arange(len(p))
            bcp = b[0]
            for jj, j in enumerate(p):            # the block's column jj holds the kept entries of A's column j, sorted by local row
                ks = [k for k in range(cp[j] - 1, cp[j + 1] - 1) if local[rv[k] - 1] >= 0]
                ks.sort(key=lambda k: local[rv[k] - 1])
                for t, k in enumerate(ks):
                    out[k] = f.fval[bcp[jj] - 1 + t]
        src = block_matrix(self.csc, self.parts, permuted)[3]
        return out[src]

    def mul(self, x):
        return self.m.mul(self.csc, x)

    def norm(self, r):
        return float(np.sqrt(self.m.dot(r, r)))

    def cg(self, b, x=None, maxiter=None, abstol=0.0, reltol=RELTOL):
        """include/esparse_hip.h, esp_cg -> (x, history, iterations, converged)"""
        n = self.n
        b = np.asarray(b, np.float64)
        maxiter = n if maxiter is None else maxiter
        u, rho = np.zeros(n), 1.0
        if x is None:
            x, r = np.zeros(n), b.copy()
        else:
            x = np.array(x, np.float64)
            r = b - self.mul(x)
        residual = self.norm(r)
        tol = reltol * residual if reltol * residual > abstol else abstol
        hist, it = [residual], 0
        with np.errstate(all="ignore"):
            while it < maxiter and not residual <= tol:
                it += 1
                c = self.ldiv(r)
                rho_prev, rho = rho, self.m.dot(c, r)
                beta = np.float64(rho) / np.float64(rho_prev)
                u = c + beta * u
                c = self.mul(u)
                alpha = np.float64(rho) / np.float64(self.m.dot(u, c))
                x = x + alpha * u
                r = r - alpha * c
                residual = self.norm(r)
                hist.append(residual)
        return x, np.array(hist), it, bool(residual <= tol)

    def bicgstabl(self, b, l=2, x=None, max_mv_products=None, abstol=0.0, reltol=RELTOL, r_shadow=None):
        """include/esparse_hip.h, esp_bicgstabl (tests/bicgstabl_model.c statement by statement)
        -> (x, history, outer iterations, matrix-vector products, converged)"""
        n = self.n
        b = np.asarray(b, np.float64)
        max_mv_products = n if max_mv_products is None else max_mv_products
        us = [np.zeros(n) for _ in range(l + 1)]
        rs = [None] * (l + 1)
        mv = 0
        if x is None:
            x, t = np.zeros(n), b.copy()
        else:
            x = np.array(x, np.float64)
            t = b - self.mul(x)
            mv = 1
        rs[0] = self.ldiv(t)
        omega = sigma = np.float64(1.0)
        rt = np.array(r_shadow, np.float64) if r_shadow is not None else rs[0].copy()
        residual = self.norm(rs[0])
        tol = reltol * residual if reltol * residual > abstol else abstol
        hist, it = [residual], 0
        with np.errstate(all="ignore"):
            while mv < max_mv_products and not residual <= tol:
                it += 1
                sigma = -omega * sigma
                for j in range(l):
                    rho = np.float64(self.m.dot(rt, rs[j]))
                    beta = rho / sigma
                    for k in range(j + 1):
                        us[k] = rs[k] - beta * us[k]
                    us[j + 1] = self.ldiv(self.mul(us[j]))
                    sigma = np.float64(self.m.dot(rt, us[j + 1]))
                    alpha = rho / sigma
                    for k in range(j + 1):
                        rs[k] = rs[k] - alpha * us[k + 1]
                    rs[j + 1] = self.ldiv(self.mul(rs[j]))
                    x = x + alpha * us[0]
                mv += 2 * l
                M = np.zeros((l + 1, l + 1))
                for i in range(l + 1):
                    for k in range(i, l + 1):
                        M[i, k] = M[k, i] = self.m.dot(rs[i], rs[k])
                gamma = np.concatenate([[0.0], self.m.gamma(M)])
                for k in range(1, l + 1):
                    us[0] = us[0] - gamma[k] * us[k]
                for k in range(1, l + 1):
                    x = x + gamma[k] * rs[k - 1]
                for k in range(1, l + 1):
                    rs[0] = rs[0] - gamma[k] * rs[k]
                omega = np.float64(gamma[l])
                residual = self.norm(rs[0])
                hist.append(residual)
        return x, np.array(hist), it, mv, bool(residual <= tol)

    @staticmethod
    def simple_norm(res):
        """norm(res) as esp_simple forms it (include/esparse_hip.h: "a fixed-order sum of squares"; csrc/precon.hip states the
        shape): the squares in chunks of 256 consecutive rows (the last one padded with +0.0), a chunk folded by the tree
        for w = 128, 64, ..., 1: s[t] = s[t] + s[t + w]; lane t of 256 adds the chunk sums t, t + 256, ... in that order to 0.0;
        the same tree over the lanes; the square root"""
        def tree(s):                     # rows of 256
            for w in (128, 64, 32, 16, 8, 4, 2, 1):
                s = s[:, :w] + s[:, w:2 * w]
            return s[:, 0]
        res = np.asarray(res, np.float64)
        nb = max(1, -(-len(res) // 256))
        sq = np.zeros(nb * 256)
        sq[:len(res)] = res * res
        part = tree(sq.reshape(nb, 256)) if len(res) else np.zeros(0)
        lanes = np.zeros(256)
        for q in range(len(part)):       # (in order: lane q % 256 meets its partials by increasing q)
            lanes[q % 256] = lanes[q % 256] + part[q]
        return float(np.sqrt(tree(lanes.reshape(1, 256))[0]))

    def simple(self, b, u=None, maxiter=100, abstol=0.0, reltol=RELTOL):
        """simple!(u, A, b; Pl) (simple_iteration.jl:21-45) -> (u, history, steps), the norm as the device forms it"""
        b = np.asarray(b, np.float64)
        u = np.zeros(self.n) if u is None else np.array(u, np.float64)
        res = self.mul(u) - b
        r0 = self.simple_norm(res)
        hist, it = [r0], 0
        with np.errstate(all="ignore"):
            for i in range(1, maxiter + 1):
                upd = self.ldiv(res)
                u = u - upd
                res = self.mul(u) - b
                r = self.simple_norm(res)
                hist.append(r)
                it = i
                if (np.float64(r) / np.float64(r0)) < reltol or r < abstol:
                    break
        return u, np.array(hist), it
