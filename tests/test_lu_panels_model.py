"""CPU: the panel schedule of LUFactorization(form="panels") pinned before any GPU run.  tests/lu_panels_modellib.py
restates it -- every entry of B by its one chain, node by node from the deepest depth up, the descendants through the update list
and then the node's own earlier positions; the two solves as row gathers in tree order -- and is held here bit for bit (a NaN equals
a NaN at the same position) to lu_modellib.Model.lu(...).fval and .ldiv, that is to iluam_model.c over B.  Also: the public
interface the form needs exists (header, ctypes table, Python arguments), which is what fails on a tree without the panel form."""
import inspect
import os
import re

import numpy as np
import pytest

import lu_modellib as L
import lu_panels_modellib as PM
from refmodel import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return L.Model(tmp_path_factory.mktemp("lu_panels_model"))


def same_bits(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def fdrand_csc(orc, nx, ny, nz, rand_mode=1):
    O = orc.fdrand(nx, ny, nz, rand_mode=rand_mode, style=orc.KIND_UPDATE)
    return tuple(np.array(a) for a in O.sparse().arrays())


def hold(model, csc, leaf_size, seed=1):
    """the restated schedule against the model on csc -> (the model's factorization, the tree)"""
    fact = model.lu(csc, leaf_size)
    tree = PM.Tree(fact)
    assert sum(tree.w) == fact.n and len(tree.start) == fact.stats["nodes"]
    fval = PM.factor(tree, fact.B)
    assert same_bits(fval, fact.fval)
    for s in (seed, seed + 1):
        v = np.random.default_rng(s).standard_normal(fact.n)
        assert same_bits(PM.ldiv(tree, fact, fval, v), fact.ldiv(v))
    return fact, tree


def test_nonsymmetric_random_pattern(model):
    fact, tree = hold(model, L.csc_of(L.random_pattern(70, False, 0.06, 5)), 4)
    assert len(tree.start) > 10 and max(len(u) for u in tree.ulist) >= 2 and len(tree.by_depth) >= 3


def test_grid_9x7(model):
    fact, tree = hold(model, L.csc_of(L.dominant(L.edges_pattern(63, L.grid_edges(9, 7)))), 4)
    assert len(tree.start) > 10 and max(len(s) for s in tree.struct) >= 7


def test_stored_zeros_and_nan(model, orc):
    """the 5 x 4 x 3 fdrand with a stored 0.0, -0.0 and NaN off-diagonal: the pattern alone decides which terms take part, so the signs
    of the zeros and the reach of the NaN are the model's"""
    cp, rv, nz = fdrand_csc(orc, 5, 4, 3)
    off = [q for j in range(len(cp) - 1) for q in range(cp[j] - 1, cp[j + 1] - 1) if rv[q] != j + 1]
    nz[off[3]], nz[off[10]], nz[off[17]] = 0.0, -0.0, np.nan
    for leaf in (4, 32):
        fact, tree = hold(model, (cp, rv, nz), leaf)
        assert np.isnan(fact.fval).any() and not np.isnan(fact.fval).all()
        assert np.signbit(PM.factor(tree, fact.B)).sum() == np.signbit(fact.fval).sum()


def test_zero_pivot_in_a_leaf(model):
    """a leaf whose second pivot cancels to 0.0 exactly: Inf appears in L, NaN follows it, both where the model has them"""
    S = L.path(12).tolil()
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = 2.0, 4.0, 1.0, 2.0       # u_11 = 2 - (4 * 0.5) = 0
    fact, _ = hold(model, L.csc_of(S.tocsc()), 4)
    assert np.isinf(fact.fval).any() or np.isnan(fact.fval).any()
    assert (fact.fval == 0.0).any()


def test_interface_exists(esp):
    """the C ABI, the ctypes table and the Python arguments of the panel form"""
    with open(os.path.join(ROOT, "include", "esparse_hip.h")) as f:
        code = f.read()
    for name in ("esp_precon_lu_create_form", "esp_precon_lu_panel_stats", "esp_debug_lu_wide_from"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in esp._lib.SIGNATURES
    assert re.search(r"#define\s+ESP_LU_COLUMNS\s+0\b", code) and re.search(r"#define\s+ESP_LU_PANELS\s+1\b", code)
    assert "form" in inspect.signature(esp.LUFactorization.__init__).parameters
    assert inspect.signature(esp.LUFactorization.__init__).parameters["form"].default == "columns"
    assert "form" in inspect.signature(esp.ExtendableSparseMatrix.solve).parameters
    assert "form" in inspect.signature(esp.solve).parameters and callable(esp.LUFactorization.panel_stats)
    lib = esp._lib.load()
    assert lib.esp_precon_lu_create_form(None, 32, 48, 1, None) == -1 and lib.esp_precon_lu_panel_stats(None, None) == -1
    assert lib.esp_debug_lu_wide_from(None, 1) == -1
