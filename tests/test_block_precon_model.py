"""CPU: the model of BlockPreconditioner (tests/block_precon_modellib.py) is held to account -- with ONE partition 0..n-1 it
is the existing models bit for bit (ldiv! of all three kinds, and its restated cg / bicgstabl loops against cg_model.c /
bicgstabl_model.c); on a block-tridiagonal matrix cut at its blocks ILUAM is exact on every block, so ldiv! solves every
block system -- and the new entry points exist without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from block_precon_modellib import BlockModel, Model, block_matrix, extract_block, increasing
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["jacobi", "ilu0", "iluam"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("block_model"))


def fdrand_csc(orc, *dims):
    O = orc.fdrand(*dims, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
    return tuple(np.array(a) for a in O.sparse().arrays())


def same(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


@pytest.mark.parametrize("kind", KINDS)
def test_single_partition_is_the_unblocked_model(model, orc, kind):
    csc = fdrand_csc(orc, 7, 6, 5)
    n = len(csc[0]) - 1
    B = BlockModel(model, orc, kind, csc, [np.arange(n)])
    P = model.precon(kind, csc, orc)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(n)
    assert same(B.ldiv(v), model.ldiv(P, csc, v))
    b = model.mul(csc, np.ones(n))
    for kw in ({"maxiter": 8}, {}):
        got, want = B.cg(b, **kw), model.cg(P, csc, b, **kw)
        assert same(got[0], want[0]) and same(got[1], want[1]) and got[2:] == want[2:]
    x0 = rng.standard_normal(n)
    got, want = B.cg(b, x=x0, maxiter=5), model.cg(P, csc, b, x=x0, maxiter=5)
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[2:] == want[2:]
    for kw in ({"l": 2, "max_mv_products": 16}, {"l": 1, "max_mv_products": 6, "x": x0}, {"l": 3, "r_shadow": rng.standard_normal(n)}):
        got, want = B.bicgstabl(b, **kw), model.bicgstabl(P, csc, b, **kw)
        assert same(got[0], want[0]) and same(got[1], want[1]) and got[2:] == want[2:]


def test_extraction_and_block_matrix_agree(orc):
    """A[part, part] by loops against SciPy's fancy indexing; B's two numberings against the same blocks"""
    csc = fdrand_csc(orc, 5, 4, 3)
    cp, rv, nz = csc
    n = len(cp) - 1
    S = sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))
    perm = np.random.default_rng(11).permutation(n)
    for parts in ([np.arange(0, n, 2), np.arange(1, n, 2)], [perm[:20], perm[20:21], perm[21:21], perm[21:]]):
        for p in parts:
            bcp, brv, bnz = extract_block(csc, p)
            W = S[p][:, p].tocsc()
            W.sort_indices()
            assert np.array_equal(bcp, W.indptr + 1) and np.array_equal(brv, W.indices + 1) and same(bnz, W.data)
        Pm = np.concatenate(parts)
        W = S[Pm][:, Pm].tolil()
        off = np.cumsum([0] + [len(p) for p in parts])
        mask = sp.block_diag([np.ones((len(p), len(p))) for p in parts if len(p)]).tocsc()
        W = sp.csc_matrix(W).multiply(mask).tocsc()
        W.sort_indices()
        bcp, brv, bnz, _ = block_matrix(csc, parts, True)
        assert np.array_equal(bcp, W.indptr + 1) and np.array_equal(brv, W.indices + 1) and same(bnz, W.data)
        if increasing(parts):
            inv = np.argsort(Pm)
            W = W[inv][:, inv].tocsc()
            W.sort_indices()
            bcp, brv, bnz, _ = block_matrix(csc, parts, False)
            assert np.array_equal(bcp, W.indptr + 1) and np.array_equal(brv, W.indices + 1) and same(bnz, W.data)
        assert off[-1] == n


def test_iluam_blocks_are_exact_on_block_tridiagonal(model, orc):
    """a block-tridiagonal matrix (tridiagonal blocks on the diagonal, diagonal couplings beside them) cut at its blocks:
    every A[part, part] is tridiagonal, ILU(0) on a tridiagonal pattern is plain LU, so u solves each block system --
    1e-10 relative against numpy.linalg.solve on the dense blocks"""
    rng = np.random.default_rng(5)
    sizes = [7, 1, 12, 5]
    n = sum(sizes)
    D = np.zeros((n, n))
    off = np.cumsum([0] + sizes)
    for a, b in zip(off[:-1], off[1:]):
        m = b - a
        D[a:b, a:b] = np.diag(4.0 + rng.random(m)) + np.diag(-1.0 - rng.random(m - 1), 1) + np.diag(-1.0 - rng.random(m - 1), -1)
    for a, b, c in zip(off[:-2], off[1:-1], off[2:]):
        m = min(b - a, c - b)
        D[a:a + m, b:b + m] += np.diag(0.3 * rng.random(m))
        D[b:b + m, a:a + m] += np.diag(0.3 * rng.random(m))
    S = sp.csc_matrix(D)
    S.sort_indices()
    csc = (S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.copy())
    parts = [np.arange(a, b) for a, b in zip(off[:-1], off[1:])]
    B = BlockModel(model, orc, "iluam", csc, parts)
    v = rng.standard_normal(n)
    u = B.ldiv(v)
    for p in parts:
        want = np.linalg.solve(D[np.ix_(p, p)], v[p])
        assert np.linalg.norm(u[p] - want) <= 1e-10 * np.linalg.norm(want)


def test_block_entry_points_declared_and_exported(esp):
    """the header declares the constant and the three new functions, the built library exports them, the package the class"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_BLOCK\s+3\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = esp._lib.load()
    for name in ("esp_precon_block_create", "esp_precon_block_matrix", "esp_debug_block_path"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert esp.ESP_PRECON_BLOCK == 3 and esp.BlockPreconditioner.KIND == 3
    with pytest.raises(TypeError):
        esp.BlockPreconditioner("not a matrix", [range(1, 3)], esp.JacobiPreconditioner)
