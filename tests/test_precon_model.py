"""CPU: the independent model of the point preconditioners and simple! (tests/precon_model.c) reproduces the reference's own
acceptance test (test/test_preconditioners.jl:10-36), and the new entry points exist without a GPU but refuse to run there."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from precon_modellib import KIND_ILU0, KIND_JACOBI, Model


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("precon_model"))


def scipy_csc(cp, rv, nz):
    n = len(cp) - 1
    return sp.csc_matrix((nz, rv - 1, cp - 1), shape=(n, n))


@pytest.mark.parametrize("rand_mode", [1, 2])
@pytest.mark.parametrize("kind,bound", [(KIND_ILU0, 4e-5), (KIND_JACOBI, 3e-4)])
def test_model_reference_acceptance(model, orc, rand_mode, kind, bound):
    """test_preconditioners.jl:10-36 on fdrand(20,20,20), b = ones: simple(A, b; Pl, maxiter = 10000, reltol = 1e-10,
    log = true) has a monotone tail and lands within 4e-5 (ILU0) / 3e-4 (Jacobi) of A \\ b."""
    O = orc.fdrand(20, 20, 20, rand_mode=rand_mode, seed=0x5EED0002, style=orc.KIND_UPDATE)
    C0 = O.sparse()   # (a view into O: O stays alive)
    cp, rv, nz = C0.arrays()
    n = len(cp) - 1
    b = np.ones(n)
    exact = spla.spsolve(scipy_csc(cp, rv, nz).tocsr(), b)
    if kind == KIND_ILU0:
        diag, idiag = C0.ilu0()
    else:
        diag, idiag = C0.jacobi(), None
    u, r, it = model.simple(kind, (cp, rv, nz), diag, idiag, b, maxiter=10000, reltol=1e-10)
    assert len(r) == it + 1
    tail = min(100, len(r) // 2)
    ratios = r[len(r) - 1 - tail:] / r[len(r) - 2 - tail:-1]
    assert np.all(ratios < 1)
    assert np.linalg.norm(u - exact) <= bound
    if kind == KIND_ILU0:
        assert it < 10000 and r[-1] / r[0] < 1e-10
    # simple! statement by statement: the last history entry is the norm of A*u - b
    res = model.mul((cp, rv, nz), u) - b
    assert r[-1] == model.norm(res)


def test_model_jacobi_ldiv_and_ilu0_aliasing(model, orc):
    """jacobi.jl:36-41 is invdiag .* v exactly; ilu0.jl:66-92 gives the same result with u === v (the device relies on it)."""
    O = orc.fdrand(12, 12, 12, rand_mode=1, seed=7, style=orc.KIND_UPDATE)
    C0 = O.sparse()
    cp, rv, nz = C0.arrays()
    n = len(cp) - 1
    v = np.random.default_rng(3).standard_normal(n)
    inv = C0.jacobi()
    assert np.array_equal(model.jacobi_ldiv(inv, v).view(np.uint64), (inv * v).view(np.uint64))
    xd, idg = C0.ilu0()
    a = model.ilu0_ldiv((cp, rv, nz), xd, idg, v)
    b = model.ilu0_ldiv((cp, rv, nz), xd, idg, v, inplace=True)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # and it is an approximate inverse: ILU0 of a diagonally dominant matrix reduces the residual of A x = v
    x = a
    A = scipy_csc(cp, rv, nz)
    assert np.linalg.norm(A @ x - v) < np.linalg.norm(v)


def test_precon_entry_points_exported(esp):
    lib = esp._lib.load()
    for name in ("esp_precon_create", "esp_precon_update", "esp_precon_ldiv", "esp_precon_destroy", "esp_simple"):
        assert hasattr(lib, name)
    assert (esp.ESP_PRECON_JACOBI, esp.ESP_PRECON_ILU0) == (0, 1)


def test_precon_python_layer_without_gpu(esp):
    with pytest.raises(TypeError):
        esp.simple(None, np.ones(3), Pl=None)          # the reference's default Pl = nothing raises
    with pytest.raises(TypeError):
        esp.ILU0Preconditioner("not a matrix")
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for cls in (esp.JacobiPreconditioner, esp.ILU0Preconditioner):
        with pytest.raises(esp.NoDeviceError):
            cls(esp.ExtendableSparseMatrix(4, 4))
