"""GPU: the vector hand-over of P.ldiv, simple, cg, bicgstabl and gmres (extendablesparse.jl_amd/precon.py) through the public API:
what is refused as x / u / out, b and r_shadow and with which message, that an accepted x / u / out is the object returned and
is updated in place, and that the host path and the CUDA path of the same call give the same bits.  One 8x8 tridiagonal matrix
(diagonal 4 .. 4.7, off-diagonals -1: Jacobi's iteration matrix has norm < 1/2, so simple! converges as well) and one Jacobi
preconditioner serve every test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 8
DIAG = 4.0 + 0.1 * np.arange(N)
DENSE = np.diag(DIAG) - np.eye(N, k=1) - np.eye(N, k=-1)
B = 1.0 + 0.25 * np.arange(N)

# name -> (the keyword of the result vector, the call); the limits are generous: every solver stops on its tolerance
CALLS = {
    "ldiv": ("out", lambda esp, A, P, b, x, **kw: P.ldiv(b, out=x)),
    "simple": ("u", lambda esp, A, P, b, x, **kw: esp.simple(A, b, u=x, Pl=P, maxiter=200)),
    "cg": ("x", lambda esp, A, P, b, x, **kw: esp.cg(A, b, Pl=P, x=x, maxiter=50)),
    "bicgstabl": ("x", lambda esp, A, P, b, x, **kw: esp.bicgstabl(A, b, l=2, Pl=P, x=x, max_mv_products=200, **kw)),
    "gmres": ("x", lambda esp, A, P, b, x, **kw: esp.gmres(A, b, Pl=P, x=x, maxiter=50)),
}
NAMES = list(CALLS)
BAD = {
    "float32": lambda: np.zeros(N, np.float32),
    "non_contiguous": lambda: np.zeros(2 * N)[::2],
    "length_n_plus_1": lambda: np.zeros(N + 1),
    "list": lambda: [0.0] * N,
}


@pytest.fixture(scope="module")
def system(esp):
    A = esp.ExtendableSparseMatrix(N, N)
    d = np.arange(1, N + 1)
    A.append(esp.ESP_UPDATE, d, d, DIAG)
    A.append(esp.ESP_UPDATE, d[:-1], d[1:], -np.ones(N - 1))
    A.append(esp.ESP_UPDATE, d[1:], d[:-1], -np.ones(N - 1))
    A.flush()
    P = esp.JacobiPreconditioner(A)
    yield A, P
    P.close()


@pytest.fixture(scope="module")
def results(esp, system):
    """every call once per placement and start: name -> {"host_given": (x handed in, what came back), "cuda_given": ..,
    "host_fresh": (None, result), "cuda_fresh": ..}"""
    import torch
    A, P = system
    out = {}
    for name, (_, call) in CALLS.items():
        hx, tx = np.zeros(N), torch.zeros(N, dtype=torch.float64, device="cuda")
        tb = torch.from_numpy(B).cuda()
        out[name] = {"host_given": (hx, call(esp, A, P, B.copy(), hx)), "cuda_given": (tx, call(esp, A, P, tb, tx)),
                     "host_fresh": (None, call(esp, A, P, B.copy(), None)), "cuda_fresh": (None, call(esp, A, P, tb, None))}
    return out


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("name", NAMES)
def test_result_vector_rejected(esp, system, name, bad):
    A, P = system
    kw, call = CALLS[name]
    with pytest.raises(ValueError) as e:
        call(esp, A, P, B.copy(), BAD[bad]())
    assert str(e.value) == "%s must be a contiguous float64 array of length n" % kw


@pytest.mark.parametrize("name", NAMES)
def test_b_of_wrong_length(esp, system, name):
    A, P = system
    with pytest.raises(ValueError) as e:
        CALLS[name][1](esp, A, P, np.ones(N + 1), None)
    assert str(e.value) == "DimensionMismatch"


@pytest.mark.parametrize("b_on, shadow_on, length, message", [
    ("host", "cuda", N, "r_shadow must live where b does"),
    ("cuda", "host", N, "r_shadow must live where b does"),
    ("host", "host", N + 1, "DimensionMismatch"),
    ("cuda", "cuda", N + 1, "DimensionMismatch"),
])
def test_r_shadow_rejected(esp, system, b_on, shadow_on, length, message):
    import torch
    A, P = system
    b = B.copy() if b_on == "host" else torch.from_numpy(B).cuda()
    rs = np.ones(length) if shadow_on == "host" else torch.ones(length, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError) as e:
        CALLS["bicgstabl"][1](esp, A, P, b, None, r_shadow=rs)
    assert str(e.value) == message


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("name", NAMES)
def test_given_vector_is_returned_and_updated_in_place(results, name, where):
    given, got = results[name][where + "_given"]
    assert got is given
    x = host(given)
    assert np.any(x != 0.0)                       # (it went in as zeros)
    if name == "ldiv":                            # invdiag .* b: one rounding for 1/d, one for the product
        assert np.allclose(x, B / DIAG, rtol=4 * np.finfo(np.float64).eps, atol=0.0)
    else:                                         # stopped at reltol = sqrt(eps) ~ 1.5e-8 of the (Jacobi-scaled) residual
        assert np.linalg.norm(B - DENSE @ x) <= 1e-6 * np.linalg.norm(B)


@pytest.mark.parametrize("start", ["given", "fresh"])
@pytest.mark.parametrize("name", NAMES)
def test_host_and_cuda_paths_agree_bitwise(results, name, start):
    h, c = host(results[name]["host_" + start][1]), host(results[name]["cuda_" + start][1])
    assert h.dtype == c.dtype == np.float64 and h.shape == c.shape == (N,)
    assert h.tobytes() == c.tobytes()
