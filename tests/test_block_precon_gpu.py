"""GPU: BlockPreconditioner on the device CSC (include/esparse_hip.h, esp_precon_block_create) against the per-block model of
tests/block_precon_modellib.py: the block matrix B bit for bit what the header says it holds, ldiv! / the ILUAM factor / x and
the whole history of cg, bicgstabl and simple! bit for bit the model's, on the identity and on the permuted path."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from bicgstabl_modellib import convdiff_triplets
from block_precon_modellib import BlockModel, Model, block_matrix, increasing
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_NOMEM, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -4, -5, -6
KINDS = ["jacobi", "ilu0", "iluam"]
KIND_ID = {"jacobi": 0, "ilu0": 1, "iluam": 2}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("block_model"))


def factorization(esp, kind):
    return {"jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}[kind]


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def same_bits(got, want):
    """bit for bit; a NaN equals a NaN at the same position"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def from_scipy(esp, S):
    """a matrix with exactly S's stored entries (explicit zeros and NaN included), through the CSC constructor"""
    S = sp.csc_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


def tridiagonal(esp, n):
    S = sp.diags([-1.0 - 0.01 * np.arange(n - 1), 4.0 + 0.001 * np.arange(n), -1.5 + 0.01 * np.arange(n - 1)], [-1, 0, 1]) if n > 1 \
        else sp.csc_matrix(np.array([[4.0]]))
    return from_scipy(esp, S)


def make(esp, A, parts, kind, force=False):
    """BlockPreconditioner over 0-based parts (the Python interface is 1-based, like A[i, j])"""
    P = esp.BlockPreconditioner(A, [np.asarray(p, np.int64) + 1 for p in parts], factorization(esp, kind))
    if force:
        assert A._d.lib.esp_debug_block_path(P._p, 1) == 0
        P.update()
    return P


def check_b(P, arrays, parts, permuted):
    assert P.path == (1 if permuted else 0)
    cp, rv, nz = P.block_matrix()
    wcp, wrv, wnz, _ = block_matrix(arrays, parts, permuted)
    assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv)
    assert np.array_equal(bits(nz), bits(wnz))          # -0.0 and NaN payloads included


def check_ldiv(P, BM, kind, permuted, seed=1):
    import torch
    n = BM.n
    v = np.random.default_rng(seed).standard_normal(n)
    want = BM.ldiv(v)
    assert same_bits(P.ldiv(v), want)
    t = torch.from_numpy(v.copy()).cuda()
    out = P.ldiv(t, out=t)                               # u aliases v
    assert out.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), want)
    h = v.copy()
    assert P.ldiv(h, out=h) is h and same_bits(h, want)
    if kind == "iluam":
        assert same_bits(P.factor(), BM.factor(permuted))
    return want


def check_all(esp, orc, model, A, parts, kind, force=False):
    arrays = host_arrays(A)
    permuted = force or not increasing(parts)
    P = make(esp, A, parts, kind, force)
    try:
        BM = BlockModel(model, orc, kind, arrays, parts)
        check_b(P, arrays, parts, permuted)
        return check_ldiv(P, BM, kind, permuted)
    finally:
        P.close()


def contiguous(n, cuts):
    return [np.arange(a, b) for a, b in zip([0] + cuts, cuts + [n])]


def shuffled(n, nparts=3, seed=17):
    perm = np.random.default_rng(seed).permutation(n)
    c = sorted(np.random.default_rng(seed + 1).choice(np.arange(1, n), nparts - 1, replace=False).tolist()) if n > nparts else []
    return [perm[a:b] for a, b in zip([0] + c, c + [n])]


# ---- matrices and partitionings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reference_partitioning_odd_even(esp, orc, model, kind):
    """fdrand 10 x 10 with test_block.jl's partitioning [1:2:n, 2:2:n]: identity path, and forced onto the permuted one"""
    A = esp.fdrand(10, 10, 1)
    n = A.n
    parts = [np.arange(0, n, 2), np.arange(1, n, 2)]
    u0 = check_all(esp, orc, model, A, parts, kind)
    u1 = check_all(esp, orc, model, A, parts, kind, force=True)
    assert same_bits(u0, u1)


@pytest.mark.parametrize("kind", KINDS)
def test_contiguous_parts_with_an_empty_and_a_single(esp, orc, model, kind):
    A = esp.fdrand(5, 4, 3)
    parts = contiguous(A.n, [17, 17, 18, 40])
    assert [len(p) for p in parts] == [17, 0, 1, 22, 20]
    u0 = check_all(esp, orc, model, A, parts, kind)
    u1 = check_all(esp, orc, model, A, parts, kind, force=True)
    assert same_bits(u0, u1)


@pytest.mark.parametrize("kind", KINDS)
def test_one_partition_is_the_unblocked_kind(esp, orc, model, kind):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    u = check_all(esp, orc, model, A, [np.arange(n)], kind)
    assert same_bits(check_all(esp, orc, model, A, [np.arange(n)], kind, force=True), u)    # (new = identity: B is the same)
    Q = factorization(esp, kind)(A)
    v = np.random.default_rng(1).standard_normal(n)
    assert same_bits(Q.ldiv(v), u)
    if kind == "iluam":
        P = make(esp, A, [np.arange(n)], kind)
        assert same_bits(P.factor(), Q.factor()) and P.levels() == Q.levels()
        P.close()
    Q.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_index_its_own_partition(esp, orc, model, kind):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    u = check_all(esp, orc, model, A, [np.array([i]) for i in range(n)], kind)
    assert same_bits(check_all(esp, orc, model, A, [np.array([i]) for i in range(n)], kind, force=True), u)
    diag = sp.csc_matrix((host_arrays(A)[2], host_arrays(A)[1] - 1, host_arrays(A)[0] - 1), shape=(n, n)).diagonal()
    v = np.random.default_rng(1).standard_normal(n)
    np.testing.assert_allclose(u, v / diag, rtol=4e-16)   # (1/d)*v (Jacobi, ILU0) or v/d (ILUAM): one or two roundings


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 257])
def test_sizes(esp, orc, model, kind, n):
    """n = 0, n = 1, and n = 257 (no multiple of any block size) in strided and in shuffled parts"""
    if n == 0:
        A = esp.ExtendableSparseMatrix(0, 0)
        for parts in ([], [np.empty(0, np.int64)]):
            P = make(esp, A, parts, kind)
            assert P.path == 0 and len(P.ldiv(np.zeros(0))) == 0
            x, log = esp.cg(A, np.zeros(0), Pl=P, log=True)
            assert log["iters"] == 0 and log["isconverged"]
            P.close()
        return
    A = tridiagonal(esp, n)
    if n == 1:
        u = check_all(esp, orc, model, A, [np.array([0])], kind)
        assert same_bits(check_all(esp, orc, model, A, [np.array([0])], kind, force=True), u)
        return
    for parts in ([np.arange(0, n, 3), np.arange(1, n, 3), np.arange(2, n, 3)], contiguous(n, [100, 200])):
        u = check_all(esp, orc, model, A, parts, kind)
        assert same_bits(check_all(esp, orc, model, A, parts, kind, force=True), u)         # the forced permuted path
    check_all(esp, orc, model, A, shuffled(n), kind)


# ---- identity-path compaction -------------------------------------------------------------------------------------------------
def test_identity_compaction_edges(esp):
    """columns that keep 0, 1, 63, 64, 65 and 129 entries, a dropped entry between every two kept ones (the lane loop below
    33 stored entries, the wave's ballot above), stored 0.0, -0.0 and a NaN among the kept values"""
    n = 300
    rng = np.random.default_rng(3)
    D = sp.lil_matrix((n, n))
    even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
    keeps = {0: 0, 2: 1, 4: 63, 6: 64, 8: 65, 10: 129, 1: 65, 3: 5}
    for j, k in keeps.items():
        mine, other = (even, odd) if j % 2 == 0 else (odd, even)
        for r in mine[:k]:
            D[r, j] = 1.0 + rng.random()
        for r in other[:k + 1]:                      # dropped, interleaved with the kept ones
            D[r, j] = -1.0 - rng.random()
    S = sp.csc_matrix(D)
    S.sort_indices()
    cp, rv, nz = S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data.copy()
    for j, special in ((4, [0.0, -0.0, np.nan]), (10, [-0.0, np.nan, 0.0]), (3, [0.0, -0.0])):
        kept = [k for k in range(cp[j] - 1, cp[j + 1] - 1) if (rv[k] - 1) % 2 == j % 2]
        for k, s in zip(kept[1::max(1, len(kept) // 4)], special):
            nz[k] = s
    A = esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, cp, rv, nz))
    arrays = host_arrays(A)
    assert np.array_equal(bits(arrays[2]), bits(nz))
    wcp = block_matrix(arrays, [even, odd], False)[0]
    assert [int(wcp[j + 1] - wcp[j]) for j in (0, 2, 4, 6, 8, 10)] == [0, 1, 63, 64, 65, 129]
    for force in (False, True):
        P = make(esp, A, [even, odd], "jacobi", force)
        check_b(P, arrays, [even, odd], force)
        P.close()


# ---- permuted path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reversed_range_and_random_permutation(esp, orc, model, kind):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    check_all(esp, orc, model, A, [np.arange(n - 1, -1, -1)], kind)
    check_all(esp, orc, model, A, shuffled(n), kind)
    check_all(esp, orc, model, A, [np.arange(0, 30), np.arange(59, 29, -1)], kind)


def arrow(esp, n, rng):
    """dense first row and column plus the diagonal"""
    r = np.arange(1, n)
    I = np.concatenate([np.arange(n), r, np.zeros(n - 1, np.int64)])
    J = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64), r])
    V = np.concatenate([10.0 + rng.random(n), 0.001 * rng.standard_normal(2 * (n - 1))])
    return from_scipy(esp, sp.csc_matrix((V, (I, J)), shape=(n, n)))


@pytest.mark.parametrize("kind", KINDS)
def test_arrow_matrix_beyond_the_column_sort(esp, orc, model, kind):
    """dense first row and column plus the diagonal, n = 4200, one shuffled partition: the first column holds 4200 entries,
    more than the per-column sort takes (4096)"""
    n = 4200
    rng = np.random.default_rng(9)
    A = arrow(esp, n, rng)
    parts = [np.random.default_rng(2).permutation(n)]
    arrays = host_arrays(A)
    P = make(esp, A, parts, kind)
    check_b(P, arrays, parts, True)
    BM = BlockModel(model, orc, kind, arrays, parts)
    v = rng.standard_normal(n)
    assert same_bits(P.ldiv(v), BM.ldiv(v))
    P.close()


# ---- updates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["strided", "shuffled"])
def test_values_only_update_equals_fresh_create(esp, orc, model, kind, which):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    parts = [np.arange(0, n, 2), np.arange(1, n, 2)] if which == "strided" else shuffled(n)
    permuted = which == "shuffled"
    P = make(esp, A, parts, kind)
    v = np.random.default_rng(6).standard_normal(n)
    u_old = P.ldiv(v)
    # (1) stored positions edited in place on the host copy, the reference's callers' way
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    assert same_bits(P.ldiv(v), u_old)                    # no update!: the values of the last update!, ILU0 included
    for step in (1, 2):
        if step == 2:                                     # (2) updates of stored positions through the buffer and a flush
            d = np.arange(1, n + 1)
            A.append(esp.ESP_UPDATE, d, d, np.full(n, 0.25))
            A.flush()
            assert same_bits(P.ldiv(v), u_new)
        P.update()
        arrays = host_arrays(A)
        F = make(esp, A, parts, kind)
        for Q in (P, F):
            check_b(Q, arrays, parts, permuted)
        BM = BlockModel(model, orc, kind, arrays, parts)
        u_new = check_ldiv(P, BM, kind, permuted, seed=6)
        assert same_bits(F.ldiv(v), u_new) and not same_bits(u_new, u_old)
        if kind == "iluam":
            assert same_bits(P.factor(), F.factor())
        F.close()
    P.close()


def test_values_only_update_after_the_scratch_route(esp, orc, model):
    """the arrow matrix at n = 4097 in one shuffled partition: a column of B holds 4097 entries, one more than the column sorts take, so
    B and src come from the flush of a scratch handle.  update! with the pattern kept gathers through that src: B, the ILUAM factor and
    ldiv! are bitwise those of a preconditioner created afresh"""
    n = 4097
    rng = np.random.default_rng(9)
    A = arrow(esp, n, rng)
    parts = [np.random.default_rng(2).permutation(n)]
    P = make(esp, A, parts, "iluam")
    assert int(np.diff(P.block_matrix()[0]).max()) == n
    v = rng.standard_normal(n)
    u_old = P.ldiv(v)
    csc = A.sparse()
    csc.nzval[:] = csc.nzval * (1.0 + 0.01 * np.random.default_rng(8).random(len(csc.nzval)))
    A._push_edits()
    P.update()
    arrays = host_arrays(A)
    F = make(esp, A, parts, "iluam")
    for Q in (P, F):
        check_b(Q, arrays, parts, True)
    u_new = P.ldiv(v)
    assert same_bits(P.factor(), F.factor()) and same_bits(u_new, F.ldiv(v)) and not same_bits(u_new, u_old)
    F.close()
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["strided", "shuffled"])
def test_pattern_change_needs_update(esp, orc, model, kind, which):
    A = esp.fdrand(5, 4, 3)
    n = A.n
    parts = [np.arange(0, n, 2), np.arange(1, n, 2)] if which == "strided" else shuffled(n)
    permuted = which == "shuffled"
    part_of = np.empty(n, np.int64)
    for ip, p in enumerate(parts):
        part_of[p] = ip
    cp, rv, _ = host_arrays(A)
    have = set(zip(rv - 1, np.repeat(np.arange(n), np.diff(cp))))             # the stored (row, column) pairs, 0-based
    j = n - 2
    inside = next(i for i in range(n) if part_of[i] == part_of[j] and (i, j) not in have)     # a new entry of B
    across = next(i for i in range(n) if part_of[i] != part_of[j] and (i, j) not in have)     # a new entry the mask drops
    P = make(esp, A, parts, kind)
    nnz_b = len(P.block_matrix()[1])
    v = np.random.default_rng(6).standard_normal(n)
    A.append(esp.ESP_UPDATE, [inside + 1, across + 1], [j + 1, j + 1], [0.5, 0.25])
    A.flush()
    with pytest.raises(esp.EspError) as e:
        P.ldiv(v)
    assert e.value.code == ESP_ERR_STATE
    with pytest.raises(esp.EspError) as e:
        esp.cg(A, v, Pl=P)
    assert e.value.code == ESP_ERR_STATE
    P.update()
    arrays = host_arrays(A)
    check_b(P, arrays, parts, permuted)
    assert len(P.block_matrix()[1]) == nnz_b + 1
    BM = BlockModel(model, orc, kind, arrays, parts)
    u = check_ldiv(P, BM, kind, permuted, seed=6)
    F = make(esp, A, parts, kind)
    assert same_bits(F.ldiv(v), u)
    F.close()
    P.close()


# ---- solvers --------------------------------------------------------------------------------------------------------------------
SOLVER = {}


def solver_matrix(esp, model, name):
    if name not in SOLVER:
        if name == "fdrand":
            A = esp.fdrand(10, 10, 1)
        else:
            I, J, V = convdiff_triplets(12, 10, 1, 1.0)
            A = esp.ExtendableSparseMatrix(120, 120)
            A.append(esp.ESP_UPDATE, I, J, V)
            A.flush()
        arrays = host_arrays(A)
        SOLVER[name] = (A, arrays, model.mul(arrays, np.ones(A.n)))
    return SOLVER[name]


def partitioning(n, which):
    return [np.arange(0, n, 2), np.arange(1, n, 2)] if which == "oddeven" else shuffled(n)


def to_device(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def to_host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def history_of(log):
    return np.concatenate([[log["r0"]], log["resnorm"]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["oddeven", "shuffled"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_cg(esp, orc, model, kind, which, where):
    """cg(A, b; Pl = BlockPreconditioner) for 8 iterations and to convergence: x and the history the model's, and x = ones to
    1e-6 relative, what test_block.jl asserts with its isapprox"""
    A, arrays, b = solver_matrix(esp, model, "fdrand")
    n = A.n
    parts = partitioning(n, which)
    P = make(esp, A, parts, kind)
    BM = BlockModel(model, orc, kind, arrays, parts)
    for kw in ({"maxiter": 8}, {}):
        bb = b if where == "host" else to_device(b)
        x, log = esp.cg(A, bb, Pl=P, log=True, **kw)
        wx, wh, wit, wconv = BM.cg(b, **kw)
        assert log["iters"] == wit and log["isconverged"] == wconv
        assert same_bits(history_of(log), wh) and same_bits(to_host(x), wx)
    assert log["isconverged"]
    x = to_host(x)
    assert np.linalg.norm(x - 1.0) <= 1e-6 * math.sqrt(n)
    x0 = np.random.default_rng(4).standard_normal(n)
    xx = x0.copy() if where == "host" else to_device(x0)
    got, log = esp.cg(A, b if where == "host" else to_device(b), Pl=P, x=xx, maxiter=5, log=True)
    wx, wh, wit, wconv = BM.cg(b, x=x0, maxiter=5)
    assert same_bits(history_of(log), wh) and same_bits(to_host(got), wx)
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["oddeven", "shuffled"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_bicgstabl(esp, orc, model, kind, which, where):
    A, arrays, b = solver_matrix(esp, model, "convdiff")
    n = A.n
    parts = partitioning(n, which)
    P = make(esp, A, parts, kind)
    BM = BlockModel(model, orc, kind, arrays, parts)
    x0 = np.random.default_rng(4).standard_normal(n)
    for kw in ({"max_mv_products": 12}, {}, {"x": x0, "max_mv_products": 9}):
        dk = dict(kw)
        if "x" in dk:
            dk["x"] = x0.copy() if where == "host" else to_device(x0)
        x, log = esp.bicgstabl(A, b if where == "host" else to_device(b), l=2, Pl=P, log=True, **dk)
        wx, wh, wit, wmv, wconv = BM.bicgstabl(b, l=2, **kw)
        assert (log["iters"], log["mvps"], log["isconverged"]) == (wit, wmv, wconv)
        assert same_bits(history_of(log), wh) and same_bits(to_host(x), wx)
    P.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["oddeven", "shuffled"])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_simple(esp, orc, model, kind, which, where):
    """five steps of simple!: u and the whole history bit for bit (the model restates the device's fixed-order norm)"""
    A, arrays, b = solver_matrix(esp, model, "fdrand")
    n = A.n
    parts = partitioning(n, which)
    P = make(esp, A, parts, kind)
    BM = BlockModel(model, orc, kind, arrays, parts)
    u0 = np.random.default_rng(12).standard_normal(n)
    uu = u0.copy() if where == "host" else to_device(u0)
    got, log = esp.simple(A, b if where == "host" else to_device(b), u=uu, Pl=P, maxiter=5, reltol=0.0, log=True)
    wu, wh, wit = BM.simple(b, u=u0, maxiter=5, reltol=0.0)
    assert wit == 5 and len(log["resnorm"]) == 6
    assert same_bits(to_host(got), wu)
    print("simple %s %s %s: largest relative difference of the norms %.3e"
          % (kind, which, where, np.max(np.abs(np.asarray(log["resnorm"]) - wh) / wh)))
    assert same_bits(log["resnorm"], wh)
    P.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def raw_create(lib, h, kind, ptr, idx, on_device=0):
    ptr = np.ascontiguousarray(ptr, np.int64)
    idx = np.ascontiguousarray(idx, np.int64)
    p = C.c_void_p()
    rc = lib.esp_precon_block_create(h, kind, len(ptr) - 1, ptr.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), on_device, C.byref(p))
    return rc, p, (lib.esp_last_error(h) or b"").decode()


def test_error_codes(esp):
    A = esp.fdrand(2, 2, 1)
    n = A.n
    assert n == 4
    lib, h = A._d.lib, A._d.h
    ok_ptr, ok_idx = [0, 2, 4], [0, 2, 1, 3]
    for kind in (-1, 3, 7):
        assert raw_create(lib, h, kind, ok_ptr, ok_idx)[0] == ESP_ERR_INVALID
    p = C.c_void_p()
    i64p = np.zeros(1, np.int64).ctypes.data_as(C.c_void_p)
    assert lib.esp_precon_block_create(h, 0, -1, i64p, i64p, 0, C.byref(p)) == ESP_ERR_INVALID            # nparts < 0
    for bad_ptr in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):                                       # a malformed part_ptr
        assert raw_create(lib, h, 0, bad_ptr, ok_idx)[0] == ESP_ERR_INVALID
    rc, _, msg = raw_create(lib, h, 0, ok_ptr, [0, 1, 7, 3])                                              # out of range
    assert rc == ESP_ERR_INVALID and "part_idx[2] = 7" in msg
    rc, _, msg = raw_create(lib, h, 0, ok_ptr, [0, -1, 2, 3])
    assert rc == ESP_ERR_INVALID and "part_idx[1] = -1" in msg
    rc, _, msg = raw_create(lib, h, 0, ok_ptr, [3, 1, 1, 0])                                              # repeated, so another is missing
    assert rc == ESP_ERR_INVALID and "index 1 appears more than once" in msg and "index 2 is in no partition" in msg
    rc, p, _ = raw_create(lib, h, 1, ok_ptr, ok_idx)
    assert rc == 0
    assert lib.esp_destroy(h) == ESP_ERR_STATE                                                             # refused while p lives
    assert lib.esp_precon_destroy(p) == 0
    # after the failed creates A still flushes and multiplies correctly
    before = host_arrays(A)
    A.append(esp.ESP_UPDATE, [1], [1], [0.5])
    A.flush()
    after = host_arrays(A)
    assert after[2][0] == before[2][0] + 0.5
    S = sp.csc_matrix((after[2], after[1] - 1, after[0] - 1), shape=(n, n))
    x = np.arange(1.0, n + 1)
    np.testing.assert_allclose(A.mul(x), S @ x, rtol=1e-15)
    # pending entries (appended through the C call, which does not flush)
    one = np.ones(1, np.int64)
    val = np.ones(1)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 1) == 0
    assert raw_create(lib, h, 0, ok_ptr, ok_idx)[0] == ESP_ERR_STATE
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    # a rectangular matrix
    R = esp.ExtendableSparseMatrix(4, 5)
    R.append(esp.ESP_UPDATE, [1], [1], [1.0])
    R.flush()
    assert raw_create(R._d.lib, R._d.h, 0, [0, 5], [0, 1, 2, 3, 4])[0] == ESP_ERR_INVALID
    # a column without a stored diagonal: ILU0 and ILUAM refuse, Jacobi gives Inf there
    M = from_scipy(esp, sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 2.0]])))
    for kind, want in ((0, 0), (1, ESP_ERR_INVALID), (2, ESP_ERR_INVALID)):
        rc, p, msg = raw_create(M._d.lib, M._d.h, kind, [0, 3], [0, 1, 2])
        assert rc == want
        if rc == 0:
            assert M._d.lib.esp_precon_destroy(p) == 0
        else:
            assert "diagonal" in msg
    # esp_destroy succeeds once the preconditioner is gone
    rc, p, _ = raw_create(lib, h, 2, ok_ptr, ok_idx)
    assert rc == 0 and lib.esp_destroy(h) == ESP_ERR_STATE
    assert lib.esp_precon_destroy(p) == 0 and lib.esp_destroy(h) == 0
    A._d.h = None


def test_device_partition_arrays(esp, orc, model):
    """on_device != 0: the partition arrays are device arrays; the result is the host form's"""
    import torch
    A = esp.fdrand(5, 4, 3)
    n = A.n
    parts = shuffled(n)
    ptr = torch.from_numpy(np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)).cuda()
    idx = torch.from_numpy(np.concatenate(parts).astype(np.int64)).cuda()
    torch.cuda.synchronize()
    lib, h = A._d.lib, A._d.h
    p = C.c_void_p()
    assert lib.esp_precon_block_create(h, 1, len(parts), C.c_void_p(ptr.data_ptr()), C.c_void_p(idx.data_ptr()), 1, C.byref(p)) == 0
    del ptr, idx                                          # the arrays were copied
    v = np.random.default_rng(1).standard_normal(n)
    u = np.empty(n)
    assert lib.esp_precon_ldiv(p, v.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), 0) == 0
    assert lib.esp_precon_destroy(p) == 0
    assert same_bits(u, BlockModel(model, orc, "ilu0", host_arrays(A), parts).ldiv(v))


def test_column_window_is_unsupported(esp):
    """ESP_ERR_UNSUPPORTED carries over: a column window on A refuses the create, and the update! of a preconditioner made before"""
    n = 8
    d = np.arange(1, n + 1)
    A = esp.ExtendableSparseMatrix(n, n)
    A.append(esp.ESP_UPDATE, d, d, np.full(n, 2.0))
    A.flush()
    P = esp.BlockPreconditioner(A, [range(1, 5), range(5, 9)], esp.JacobiPreconditioner)
    lib, h = A._d.lib, A._d.h
    assert lib.esp_reset(h) == 0                                       # a window is exclusive when declared on an empty matrix
    assert lib.esp_set_column_window(h, 1, 4) == 0
    one = np.arange(1, 5, dtype=np.int64)
    val = np.full(4, 2.0)
    assert lib.esp_append_host(h, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), None,
                               esp.ESP_UPDATE, 0, 4) == 0
    z, ch = C.c_int64(), C.c_int32()
    assert lib.esp_flush(h, 0, C.byref(z), C.byref(ch)) == 0
    for kind in (0, 1, 2):
        rc, _, msg = raw_create(lib, h, kind, [0, 4, 8], np.arange(8))
        assert rc == ESP_ERR_UNSUPPORTED and "window" in msg
    assert lib.esp_precon_update(P._p) == ESP_ERR_UNSUPPORTED
    v = np.ones(n)
    assert lib.esp_precon_ldiv(P._p, v.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), 0) == ESP_ERR_STATE
    P.close()


def test_absurd_nparts_is_an_error_code(esp):
    A = esp.fdrand(2, 2, 1)
    p = C.c_void_p()
    z = np.zeros(1, np.int64).ctypes.data_as(C.c_void_p)
    assert A._d.lib.esp_precon_block_create(A._d.h, 0, 2 ** 62, z, z, 0, C.byref(p)) == ESP_ERR_NOMEM


@pytest.mark.parametrize("which", ["slabs", "strided", "shuffled"])
def test_iluam_levels_are_the_maximum_over_the_blocks(esp, which):
    """one factorization and one solve for all blocks: every schedule has as many levels as the deepest block's own, not their sum"""
    from block_precon_modellib import extract_block
    from iluam_modellib import level_schedules
    A = esp.fdrand(6, 5, 4)
    n = A.n
    parts = {"slabs": contiguous(n, [30, 50, 90]), "strided": [np.arange(0, n, 2), np.arange(1, n, 2)], "shuffled": shuffled(n)}[which]
    arrays = host_arrays(A)
    per_block = [[int(lev.max()) + 1 for lev in level_schedules(*extract_block(arrays, p)[:2])] for p in parts]
    P = make(esp, A, parts, "iluam")
    U = esp.ILUAMPreconditioner(A)
    assert P.levels() == tuple(max(b[k] for b in per_block) for k in range(3))
    assert all(P.levels()[k] < sum(b[k] for b in per_block) for k in range(3))
    if which == "slabs":
        assert all(a < b for a, b in zip(P.levels(), U.levels()))
    P.close()
    U.close()


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_python_interface(esp):
    A = esp.fdrand(10, 10, 1)
    n = A.n
    with pytest.raises(TypeError) as e:
        esp.BlockPreconditioner(A, [range(1, n + 1, 2), range(2, n + 1, 2)])
    assert "LUFactorization" in str(e.value) and "not on the device" in str(e.value)
    with pytest.raises(TypeError):
        esp.BlockPreconditioner(A, [range(1, n + 1)], "ilu0")
    b = A.mul(np.ones(n))
    for fact in (esp.JacobiPreconditioner, esp.ILU0Preconditioner, esp.ILUAMPreconditioner):
        P = esp.BlockPreconditioner(A, [range(1, n + 1, 2), range(2, n + 1, 2)], fact)     # test_block.jl's [1:2:n, 2:2:n]
        assert P.path == 0
        sol = esp.cg(A, b, Pl=P)
        assert np.linalg.norm(sol - 1.0) <= 1e-6 * math.sqrt(n)
        assert np.array_equal(bits(esp.bicgstabl(A, b, Pl=P)), bits(esp.bicgstabl(A, b, Pl=P)))
        P.update()
        P.close()
        with pytest.raises(ValueError):
            P.ldiv(b)
    Q = esp.BlockPreconditioner(A, factorization=esp.ILU0Preconditioner)                   # partitioning = nothing: [1:n]
    U = esp.ILU0Preconditioner(A)
    assert Q.path == 0 and np.array_equal(bits(Q.ldiv(b)), bits(U.ldiv(b)))
    with pytest.raises(esp.EspError):
        esp.BlockPreconditioner(A, [range(1, n)], esp.JacobiPreconditioner)                # one index missing
    Q.close()
    U.close()
