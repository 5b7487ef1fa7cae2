"""A numpy model of the PULL order of the stencil generator (fdrand!, sprand.jl:87-124): what lands in column l, in call order,
written down from the column's own node and its three lower neighbours alone -- the order the fused pair kernel
(csrc/local_x.hip, pair_gen_pred_k) forms a column's updates in.

For column l, with node g = l - 1 at (i, j, k) (1-based), nxy = nx ny:

    k>1 : v=vz(g-nxy): (l-nxy,-v) (l,+v)      j>1 : v=vy(g-nx): (l-nx,-v) (l,+v)      i>1 : v=vx(g-1): (l-1,-v) (l,+v)
    i<nx: v=vx(g): (l+1,-v) (l,+v)            i==1||i==nx: (l, draw1 hy hz)
    j<ny: v=vy(g): (l+nx,-v) (l,+v)           ny>2&&(j==1||j==ny): (l, draw3 hx hz)
    k<nz: v=vz(g): (l+nxy,-v) (l,+v)          nz>2&&(k==1||k==nz): (l, draw5 hx hy)
    vx(g)=draw0(g) hy hz/hx   vy(g)=draw2(g) hx hz/hy   vz(g)=draw4(g) hx hy/hz

draw q of node g is the generator's uniform number with counter 6 g + q (rand_mode 2), 0.1 + it (1) or 1.0 (0).  The model takes
the draws from a caller's function so that it needs nothing but numpy; tests hand it the oracle's orc_uniform.
"""
import numpy as np

GRIDS = [(5, 4, 3), (7, 3, 1), (6, 2, 5), (6, 5, 2), (1, 6, 5), (2, 5, 4), (9, 1, 1), (4, 1, 3), (3, 3, 3), (1, 1, 1), (2, 2, 2)]
MAX_RUN = 12


def draws(uniform, N, rand_mode, seed):
    """(N, 6) array: draw q of node g"""
    if rand_mode == 0:
        return np.ones((N, 6))
    d = np.array([[uniform(seed, 6 * g + q) for q in range(6)] for g in range(N)], np.float64).reshape(N, 6)
    return 0.1 + d if rand_mode == 1 else d


def node_of(g, nx, ny):
    return g % nx + 1, (g // nx) % ny + 1, g // (nx * ny) + 1


def column_pull(l, nx, ny, nz, D):
    """the updates of column l (1-based) in call order: list of (row, value); D = draws(...)"""
    nxy = nx * ny
    g = l - 1
    i, j, k = node_of(g, nx, ny)
    hx, hy, hz = 1.0 / nx, 1.0 / ny, 1.0 / nz

    def vx(q):
        return D[q, 0] * hy * hz / hx

    def vy(q):
        return D[q, 2] * hx * hz / hy

    def vz(q):
        return D[q, 4] * hx * hy / hz

    out = []
    if k > 1:
        v = vz(g - nxy)
        out += [(l - nxy, -v), (l, v)]
    if j > 1:
        v = vy(g - nx)
        out += [(l - nx, -v), (l, v)]
    if i > 1:
        v = vx(g - 1)
        out += [(l - 1, -v), (l, v)]
    if i < nx:
        v = vx(g)
        out += [(l + 1, -v), (l, v)]
    if i == 1 or i == nx:
        out.append((l, D[g, 1] * hy * hz))
    if j < ny:
        v = vy(g)
        out += [(l + nx, -v), (l, v)]
    if ny > 2 and (j == 1 or j == ny):
        out.append((l, D[g, 3] * hx * hz))
    if k < nz:
        v = vz(g)
        out += [(l + nxy, -v), (l, v)]
    if nz > 2 and (k == 1 or k == nz):
        out.append((l, D[g, 5] * hx * hy))
    return out


def column_sorted(pull):
    """the run as the bucket kernel folds it: by (row, call order) -- the off-diagonal rows hold one update each"""
    return sorted(pull, key=lambda rv: rv[0])  # (stable)


def stream_by_column(I, J, V, N):
    """the oracle's stream filtered by column, call order kept: list (per column, 1-based l at index l - 1) of (row, value)"""
    cols = [[] for _ in range(N)]
    for r, c, v in zip(I.tolist(), J.tolist(), V.tolist()):
        cols[c - 1].append((r, v))
    return cols


def bits(pairs):
    return [(r, np.float64(v).view(np.uint64).item()) for r, v in pairs]
