"""CPU: the normative model of LUFactorization (tests/lu_model.c: nested dissection, the tree, the predicted fill; the numerics are
iluam_model.c's over the filled matrix) is held to the properties the rule promises -- a permutation, contiguous nodes, ancestors
behind descendants, separators that separate, a pattern containing the fill of a dense elimination without pivoting -- to recorded
counts, to numpy.linalg.solve, and to the reference's own acceptance tests (test/test_backslash.jl, test/test_lu.jl).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lu_modellib as L
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return L.Model(tmp_path_factory.mktemp("lu_model"))


def fdrand_csc(orc, nx, ny, nz, rand_mode=1):
    O = orc.fdrand(nx, ny, nz, rand_mode=rand_mode, style=orc.KIND_UPDATE)
    return tuple(np.array(a) for a in O.sparse().arrays())


def scipy_of(csc):
    n = len(csc[0]) - 1
    return sp.csc_matrix((csc[2], csc[1] - 1, csc[0] - 1), shape=(n, n))


def table(orc):
    """the matrices of the issue's prototype table, with the leaf size each is run at"""
    return {"fd10x10x10": (fdrand_csc(orc, 10, 10, 10), 16), "fd20x20": (fdrand_csc(orc, 20, 20, 1), 8),
            "path100": (L.csc_of(L.path(100)), 8), "diagonal": (L.csc_of(sp.identity(50) * 2.0), 32),
            "blockdiag": (L.csc_of(L.block_diagonal()), 4), "random300": (L.csc_of(L.random_pattern(300, False, 0.01, 7)), 32),
            "arrow200": (L.csc_of(L.arrow(200)), 32)}


def seeded(n_cases=6):
    out = {}
    for k in range(n_cases):
        n = (40, 97, 150, 211, 300, 64)[k]
        out["seed%d" % k] = (L.csc_of(L.random_pattern(n, k % 2 == 0, (0.05, 0.02, 0.015, 0.01, 0.008, 0.2)[k], 100 + k)), (4, 8, 16, 32, 32, 8)[k])
    return out


def neighbours(csc):
    A = scipy_of(csc)
    G = sp.csr_matrix(((A != 0) + (A != 0).T).astype(np.int8))       # (the tests' values are non-zero: the stored pattern)
    G.setdiag(0)
    G.eliminate_zeros()
    return G


def check_tree(model, csc, leaf, max_depth=48):
    n = len(csc[0]) - 1
    c, level, root, nstart, nsize, anc, rounds, nodes = model.nested_dissection(csc, leaf, max_depth)
    assert np.array_equal(np.sort(c), np.arange(n))                                   # a permutation
    pos = np.empty(n, np.int64)
    pos[c] = np.arange(n)
    anc = anc[:(max_depth + 1) * n].reshape(max_depth + 1, n)
    node = {}
    for v in range(n):
        node.setdefault((int(level[v]), int(root[v])), []).append(pos[v])
    assert len(node) == nodes
    for (d, r), ps in node.items():                                                   # every node is contiguous in c
        ps = np.sort(ps)
        assert np.array_equal(ps, np.arange(ps[0], ps[0] + len(ps)))
        assert np.all(nstart[ps] == ps[0]) and np.all(nsize[ps] == len(ps))
    first = {k: min(ps) for k, ps in node.items()}
    G = neighbours(csc)
    for v in range(n):
        for e in range(level[v]):                                                     # every ancestor lies behind its descendants
            a = (e, int(anc[e, v]))
            assert a in first and first[a] > pos[v]
        assert anc[level[v], v] == root[v]
    # no edge joins the two sides of a split: neighbours of different levels are ancestor and descendant, neighbours of one level
    # share their node
    for u in range(n):
        for v in G.indices[G.indptr[u]:G.indptr[u + 1]]:
            lo = min(level[u], level[v])
            assert anc[lo, u] == anc[lo, v]
    return c, level, rounds


def check_fill(model, csc, leaf, max_depth=48):
    F = model.lu(csc, leaf, max_depth)
    n = F.n
    P = L.pattern_of(F.B[0], F.B[1])
    assert np.array_equal(P, P.T)
    D = L.dense_of(csc)[np.ix_(F.c, F.c)]
    LU = L.dense_lu_nopivot(D)
    assert not (LU != 0.0)[~P].any()                                                  # the pattern contains the elimination's fill
    assert P[(D != 0.0)].all()
    B = L.dense_of(F.B)
    assert np.array_equal(bits(B[P]), bits(D[P]))                                     # A[c,c] where stored, +0.0 elsewhere
    return F, int((LU != 0.0).sum())


@pytest.mark.parametrize("name", ["fd10x10x10", "fd20x20", "path100", "diagonal", "blockdiag", "random300", "arrow200"])
def test_table_matrices(model, orc, name):
    csc, leaf = table(orc)[name]
    check_tree(model, csc, leaf)
    F, true_fill = check_fill(model, csc, leaf)
    print("%s: nnz(A) = %d, nnz(B) = %d, true fill %d, %s" % (name, len(csc[1]), F.stats["nnz"], true_fill, F.stats))


@pytest.mark.parametrize("name", sorted(seeded()))
def test_seeded_patterns(model, name):
    csc, leaf = seeded()[name]
    check_tree(model, csc, leaf)
    check_fill(model, csc, leaf)


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_depth_cap(model, orc, max_depth):
    csc = fdrand_csc(orc, 6, 5, 4)
    c, level, rounds = check_tree(model, csc, 4, max_depth)
    assert rounds == max_depth + 1 and level.max() == max_depth
    F, _ = check_fill(model, csc, 4, max_depth)
    if max_depth == 0:
        assert F.stats["nnz"] == F.n * F.n and np.array_equal(c, np.arange(F.n))      # one dense leaf in index order


def test_fixed_counts(model, orc):
    """the numbers of the rule: no fill for the arrow and the diagonal matrix; fdrand 10 x 10 x 10 with leaf_size 16 as recorded from
    lu_model.c (the key decides the roots), below the natural ordering's complete fill of 182 818"""
    for S in (L.arrow(200), sp.identity(50) * 2.0):
        csc = L.csc_of(S)
        assert model.lu(csc).stats["nnz"] == len(csc[1])
    st = model.lu(fdrand_csc(orc, 10, 10, 10), 16).stats
    print("fdrand 10x10x10, leaf_size 16:", st)
    assert (st["rounds"], st["deepest"], st["nnz"]) == (8, 7, 78308)
    assert st["nnz"] < 182818


def dominant_nonsymmetric(n=60, seed=31):
    """the matrix of test_iluk_model.py: seeded, strictly diagonally dominant by columns and by rows, non-symmetric"""
    rng = np.random.default_rng(seed)
    M = np.where(rng.random((n, n)) < 0.08, rng.standard_normal((n, n)), 0.0)
    np.fill_diagonal(M, 0.0)
    M[np.arange(1, n), np.arange(n - 1)] = -1.0
    np.fill_diagonal(M, 1.0 + np.maximum(np.abs(M).sum(0), np.abs(M).sum(1)))
    return L.csc_of(sp.csc_matrix(M))


@pytest.mark.parametrize("which", ["fd5x4x3", "fd10x10x10", "dominant"])
def test_direct_solve_accuracy(model, orc, which):
    """|b - A x| / |b| is at most 16 times numpy.linalg.solve's for the same system: the margin of
    test_iluk_model.py::test_complete_fill_is_a_direct_solve, for its reason (another elimination order, no pivoting; the growth
    factor of a diagonally dominant matrix is at most 2)"""
    csc = {"fd5x4x3": lambda: fdrand_csc(orc, 5, 4, 3), "fd10x10x10": lambda: fdrand_csc(orc, 10, 10, 10),
           "dominant": dominant_nonsymmetric}[which]()
    n = len(csc[0]) - 1
    F = model.lu(csc)
    A = scipy_of(csc).toarray()
    b = np.random.default_rng(5).standard_normal(n)
    x = F.solve(b)
    ref = np.linalg.solve(A, b)
    r = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    r_ref = np.linalg.norm(b - A @ ref) / np.linalg.norm(b)
    print("direct solve %s: n = %d, nnz(B) = %d of %d, |b - A x|/|b| = %.3e, numpy.linalg.solve %.3e" % (which, n, F.stats["nnz"], len(csc[1]), r, r_ref))
    assert r <= 16 * r_ref
    assert np.array_equal(bits(F.ldiv(b.copy(), inplace=True)), bits(x))


# ---- the reference's acceptance tests, replayed on the model ---------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(100, 1, 1), (20, 20, 1), (10, 10, 10)])
def test_reference_backslash(model, orc, grid):
    """test/test_backslash.jl: fdrand(k, l, m; rand = () -> 1), x = ones, b = A*x, norm(A \\ b - x) <= 10 sqrt(eps)"""
    csc = fdrand_csc(orc, *grid, rand_mode=0)
    A = scipy_of(csc)
    x = np.ones(A.shape[0])
    assert np.linalg.norm(model.lu(csc).solve(A @ x) - x) <= 10.0 * np.sqrt(EPS)


def plus_diagonal(csc, add):
    cp, rv, nz = (np.array(a) for a in csc)
    for j in range(len(cp) - 1):
        q = cp[j] - 1 + int(np.searchsorted(rv[cp[j] - 1:cp[j + 1] - 1], j + 1))
        assert rv[q] == j + 1
        nz[q] += add
    return cp, rv, nz


@pytest.mark.parametrize("grid", [(10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu1(model, orc, grid):
    """test/test_lu.jl:7-31: factor, solve, add 1.0 to every diagonal entry, update!, solve again; both answers agree with a dense
    solve to 100 sqrt(eps), relative"""
    csc = fdrand_csc(orc, *grid, rand_mode=0)
    b = np.random.default_rng(11).random(len(csc[0]) - 1)
    F = model.lu(csc)
    x1 = F.solve(b)
    csc2 = plus_diagonal(csc, 1.0)
    F.update(csc2)
    assert F.builds == 1                                                              # the pattern kept: the values only
    x2 = F.solve(b)
    for x, a in ((x1, csc), (x2, csc2)):
        ref = np.linalg.solve(scipy_of(a).toarray(), b)
        assert np.linalg.norm(ref - x) / np.linalg.norm(ref) <= 100.0 * np.sqrt(EPS)
    fresh = model.lu(csc2)
    assert np.array_equal(bits(fresh.fval), bits(F.fval)) and np.array_equal(bits(fresh.solve(b)), bits(x2))


def off_diagonals(csc, by=1.0e-4):
    """test_lu.jl:38-41: A[i, i+3] -= by, A[i-3, i] -= by for i = 4 .. n-3 (1-based): the same positions, each lowered twice where
    both statements name it"""
    A = sp.lil_matrix(scipy_of(csc))
    n = A.shape[0]
    stored = set(zip(*scipy_of(csc).nonzero()))
    new = {}
    for i in range(3, n - 3):
        for (r, c) in ((i, i + 3), (i - 3, i)):
            new[(r, c)] = new.get((r, c), A[r, c] if (r, c) in stored else 0.0) - by
    M = sp.coo_matrix(scipy_of(csc))
    keys = {(int(r), int(c)): v for r, c, v in zip(M.row, M.col, M.data)}
    keys.update(new)
    rc = sorted(keys, key=lambda t: (t[1], t[0]))
    S = sp.csc_matrix(([keys[t] for t in rc], ([t[0] for t in rc], [t[1] for t in rc])), shape=(n, n))
    return L.csc_of(S)


@pytest.mark.parametrize("grid", [(10, 10, 10), (25, 40, 1), (1000, 1, 1)])
def test_reference_lu2(model, orc, grid):
    """test/test_lu.jl:33-45: after the off-diagonal edit (a pattern change) and lu!, every component of the new solution exceeds
    the old one"""
    csc = fdrand_csc(orc, *grid, rand_mode=0)
    b = np.random.default_rng(12).random(len(csc[0]) - 1)
    F = model.lu(csc)
    x1 = F.solve(b)
    csc2 = off_diagonals(csc)
    assert len(csc2[1]) > len(csc[1])
    F.update(csc2)
    assert F.builds == 2                                                              # everything anew
    assert np.all(x1 < F.solve(b))


def test_a_missing_diagonal_is_refused(model):
    csc = L.csc_of(sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 0.0]])))
    with pytest.raises(ValueError):
        model.lu(csc)


def test_lu_entry_points_declared_and_exported(esp):
    """the header declares the constant and the calls, the binding table holds them, the package exports the interface"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    assert re.search(r"^#define\s+ESP_PRECON_LU\s+9\s*$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = esp._lib.load()
    for name in ("esp_precon_lu_create", "esp_precon_lu_perm", "esp_precon_lu_tree", "esp_precon_lu_matrix", "esp_precon_lu_stats",
                 "esp_nested_dissection", "esp_debug_lu_fill_cap"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    assert esp.ESP_PRECON_LU == 9 and esp.LUFactorization.KIND == 9 and esp.SparspakLU is esp.LUFactorization
    assert esp.issolver(esp.LUFactorization)
    for cls in (esp.JacobiPreconditioner, esp.ILU0Preconditioner, esp.ILUAMPreconditioner, esp.ILUKPreconditioner, esp.ILUTPreconditioner,
                esp.BlockPreconditioner, esp.ColoredPreconditioner, esp.ParallelILU0Preconditioner, esp.SPAIPreconditioner,
                esp.AMGPreconditioner, esp.RS_AMGPreconditioner):
        assert not esp.issolver(cls)
    for call in (esp.lu, esp.nested_dissection, lambda A: esp.lu_(A, A), lambda A: esp.factorize_(A, A), lambda A: esp.solve(A, None)):
        with pytest.raises(TypeError):
            call("not a matrix")


def test_factor_form_entry_points_declared_and_exported(esp):
    """the hook and the read-out of ILUAM's two forms: declared in the header, bound, exported, and on every class with .launches()"""
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = esp._lib.load()
    for name in ("esp_debug_iluam_form", "esp_debug_last_iluam_form"):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code) and name in esp._lib.SIGNATURES and hasattr(lib, name)
    form = C.c_int32(7)
    assert lib.esp_debug_iluam_form(None, 1) == -1 and lib.esp_debug_last_iluam_form(None, C.byref(form)) == -1 and form.value == 7
    with_launches = [cls for cls in (esp.ILUAMPreconditioner, esp.BlockPreconditioner, esp.ILUKPreconditioner, esp.ColoredPreconditioner,
                                     esp.ParallelILU0Preconditioner, esp.ILUTPreconditioner, esp.LUFactorization)]
    for cls in with_launches:
        assert callable(cls.launches) and callable(cls.debug_factor_form) and callable(cls.last_factor_form)
    for cls in (esp.JacobiPreconditioner, esp.ILU0Preconditioner, esp.AMGPreconditioner, esp.SPAIPreconditioner):
        assert not hasattr(cls, "launches") and not hasattr(cls, "debug_factor_form") and not hasattr(cls, "last_factor_form")
