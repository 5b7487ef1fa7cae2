"""The panel schedule of LUFactorization(form="panels") restated in Python (test infrastructure): the tree tables read
off the model's B (lu_modellib.LuFact), every entry of B evaluated by its ONE chain node by node from the deepest depth up, and the two
solves as row gathers in ILUAM's orders, depth by depth.  tests/test_lu_panels_model.py holds it bit for bit to the model's fval and
ldiv (iluam_model.c over B).  Nothing here knows of the device code; np.float64 scalars round every product, difference and quotient
on their own and let Inf and NaN through."""
import numpy as np


class Tree:
    """the nodes of fact's dissection tree in position order: .start, .w, .struct (positions, ascending), .depth, .ulist (the nodes
    whose struct holds one of K's positions, ascending); .nodeof[position]; .by_depth[d] = the nodes of depth d, ascending"""

    def __init__(self, fact):
        n = fact.n
        bcp, brv, _ = fact.B
        self.n = n
        self.start, self.w, self.struct, self.depth = [], [], [], []
        self.nodeof = np.zeros(n, np.int64)
        k = 0
        while k < n:
            w = int(fact.nsize[k])
            assert fact.nstart[k] == k and w > 0
            rows = brv[bcp[k] - 1:bcp[k + 1] - 1] - 1
            self.nodeof[k:k + w] = len(self.start)
            self.start.append(k)
            self.w.append(w)
            self.struct.append([int(r) for r in rows if r >= k + w])
            self.depth.append(int(fact.level[fact.c[k]]))
            k += w
        m = len(self.start)
        self.sets = [set(s) for s in self.struct]
        self.ulist = [[] for _ in range(m)]
        for J in range(m):
            for K in sorted({int(self.nodeof[p]) for p in self.struct[J]}):
                self.ulist[K].append(J)
        deepest = max(self.depth) if m else -1
        self.by_depth = [[K for K in range(m) if self.depth[K] == d] for d in range(deepest + 1)]

    def positions(self, K):
        return list(range(self.start[K], self.start[K] + self.w[K]))


def factor(tree, B):
    """fval in B's position order: L scaled below the diagonal, U on and above it"""
    bcp, brv, bnz = B
    where = {(int(brv[q] - 1), j): q for j in range(tree.n) for q in range(bcp[j] - 1, bcp[j + 1] - 1)}
    val = np.array(bnz, np.float64, copy=True)

    def at(k, j):
        return val[where[(k, j)]]

    with np.errstate(all="ignore"):
        for d in range(len(tree.by_depth) - 1, -1, -1):
            for K in tree.by_depth[d]:
                own = tree.positions(K)
                rows = own + tree.struct[K]
                for mi, m in enumerate(own):
                    # the entries whose chain ends at m: row m of U from the diagonal on, then column m of L
                    for k, j in [(m, r) for r in rows[mi:]] + [(r, m) for r in rows[mi + 1:]]:
                        t = at(k, j)
                        for J in tree.ulist[K]:
                            if k in tree.sets[J] and j in tree.sets[J]:          # the predicate: never a product with a zero
                                for i in tree.positions(J):
                                    t = t - at(i, j) * at(k, i)                  # u_ij * l_ki
                        for i in own[:mi]:
                            t = t - at(i, j) * at(k, i)
                        if k > j:
                            t = t / at(j, j)
                        val[where[(k, j)]] = t
    return val


def ldiv(tree, fact, fval, v):
    """u[c] = U \\ (L \\ v[c]) on the factor fval (B's position order)"""
    bcp, brv, _ = fact.B
    n = tree.n
    v = np.asarray(v, np.float64)
    if n == 0:
        return v.copy()
    where = {(int(brv[q] - 1), j): q for j in range(n) for q in range(bcp[j] - 1, bcp[j + 1] - 1)}
    b = v[fact.c]
    y = np.zeros(n)
    with np.errstate(all="ignore"):
        for d in range(len(tree.by_depth) - 1, -1, -1):      # forward: the deepest depth first
            for K in tree.by_depth[d]:
                own = tree.positions(K)
                for ji, j in enumerate(own):
                    acc = np.float64(0.0)
                    for J in tree.ulist[K]:
                        if j in tree.sets[J]:
                            for k in tree.positions(J):
                                acc = acc - fval[where[(j, k)]] * y[k]
                    for k in own[:ji]:
                        acc = acc - fval[where[(j, k)]] * y[k]
                    y[j] = acc + b[j]                         # the right-hand side last
        x = np.zeros(n)
        for d in range(len(tree.by_depth)):                   # backward: depth 0 first
            for K in tree.by_depth[d]:
                own = tree.positions(K)
                for ji in range(len(own) - 1, -1, -1):
                    j = own[ji]
                    acc = y[j]
                    for i in reversed(tree.struct[K]):        # the stored i > j descending
                        acc = acc - fval[where[(j, i)]] * x[i]
                    for i in reversed(own[ji + 1:]):
                        acc = acc - fval[where[(j, i)]] * x[i]
                    x[j] = acc / fval[where[(j, j)]]
    out = np.empty(n)
    out[fact.c] = x
    return out
