"""GPU: the pass-count edges of the library's single-segment LSD sorts (csrc/partition.hip, sort_segment_lsd), each through the
public API of the site that sorts, bit for bit against the CPU oracle or the model the site's own tests use.

The sort runs 8 key bits per pass, the last pass what is left, and ping-pongs between two buffers: the parity of the pass count
decides which half holds the result, and the last pass may be a short digit.  So every site is taken at a bit count of 8 (one
full pass) and 9 (a full pass and a 1-bit pass), and at 16 and 17 where that is cheap.

Held elsewhere already: build_csr's row sort at 8, 9, 16 and 17 row bits is tests/test_consumers_gpu.py::test_mul_row_index
[mul_m256 / mul_m257 / mul_m65536 / mul_m65537] (consumer_cases.MUL_M), against the oracle's product; the AMG aggregates and the
coarse inverse into host and device memory, against the model, are test_amg_gpu.py's check_hierarchy and
test_inspection_into_device_memory."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import coloring_modellib
import iluam_modellib
import lu_modellib
from consumer_cases import bits_for
from refmodel import assert_csc_equal, bits

pytestmark = pytest.mark.gpu

GENERAL = 2          # ESP_PATH_GENERAL: the pending buffer sorted by sort_pending_lsd on all its (column, row) bits
SET, UPDATE, RAWUPDATE = 0, 1, 2


def passes(nbits):
    return -(-nbits // 8)


def same_bits(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def host_arrays(A):
    return tuple(np.array(a, copy=True) for a in A.sparse().arrays())


def from_scipy(esp, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    return esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(n, n, S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1,
                                                          S.data.astype(np.float64)))


# ---- the general flush: sort_pending_lsd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,sort_bits", [(16, 16, 8), (16, 32, 9), (256, 256, 16), (256, 512, 17)])
def test_general_flush(esp, orc, m, n, sort_bits):
    """KeyLayout (csrc/common.hpp): rb = bits_for(m), cb = bits_for(n), sort_bits() = rb + cb.  Three flushes of mixed kinds with
    duplicates: onto the empty matrix, then twice joined with the stored one (after an odd pass count the handle's buffers have
    changed places)."""
    assert bits_for(m) + bits_for(n) == sort_bits
    rng = np.random.default_rng([41, m, n])
    A = esp.ExtendableSparseMatrix(m, n)
    A.debug_force_path(GENERAL)
    O = orc.ExtendableSparseMatrix(m, n)
    pool = np.array([0.0, -0.0, 1.5, -1.5, 3.25])
    for flush in range(3):
        cnt = 3000
        kinds = rng.integers(0, 3, cnt).astype(np.uint8)
        I, J = rng.integers(1, m + 1, cnt), rng.integers(1, n + 1, cnt)
        I[:2], J[:2] = (1, m), (1, n)                              # the lowest and the highest key
        V = np.where(rng.random(cnt) < 0.3, rng.choice(pool, cnt), rng.standard_normal(cnt))
        A.append(0, I, J, V, kinds=kinds)
        O.apply(kinds, I, J, V)
        A.flush()
        O.flush()
        assert A.debug_last_path() == GENERAL
        assert_csc_equal(A.sparse().arrays(), O.arrays(), "flush %d" % flush)


# ---- ILUAM's schedules: build_schedule ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iluam_model(tmp_path_factory):
    return iluam_modellib.Model(tmp_path_factory.mktemp("sort_driver_iluam"))


@pytest.mark.parametrize("n", [256, 257])
def test_iluam_chain(esp, iluam_model, n):
    """a lower bidiagonal chain: n levels of one node in the factorization's and the forward schedule -- 256 levels sort on 8 bits,
    257 on 9 --, one level in the backward schedule (1 bit)"""
    rng = np.random.default_rng([43, n])
    A = from_scipy(esp, sp.diags([rng.standard_normal(n - 1), 2.0 + rng.random(n)], [-1, 0]))
    arrays = host_arrays(A)
    P = esp.ILUAMPreconditioner(A)
    try:
        want_levels = tuple(int(l.max()) + 1 for l in iluam_modellib.level_schedules(arrays[0], arrays[1]))
        assert P.levels() == want_levels and max(want_levels) == n and bits_for(n) == (8 if n == 256 else 9)
        f, diag = iluam_model.factor(arrays)
        assert same_bits(P.factor(), f)
        v = rng.standard_normal(n)
        assert same_bits(P.ldiv(v), iluam_model.ldiv(arrays, f, diag, v))
    finally:
        P.close()


# ---- the multicolour ordering: color_maps -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def color_model(tmp_path_factory):
    return coloring_modellib.Model(tmp_path_factory.mktemp("sort_driver_coloring"))


@pytest.mark.parametrize("n", [256, 257])
def test_coloring_complete_graph(esp, color_model, n):
    """the complete graph on n vertices (a dense pattern): n colours, sorted on 8 bits (256) and on 9 (257)"""
    rng = np.random.default_rng([45, n])
    M = 0.01 * rng.standard_normal((n, n))
    np.fill_diagonal(M, 2.0 + rng.random(n))
    A = from_scipy(esp, sp.csc_matrix(M))
    arrays = host_arrays(A)
    assert len(arrays[1]) == n * n
    col = color_model.coloring(arrays[0], arrays[1])
    assert col.ncolors == n
    P = esp.ColoredPreconditioner(A, esp.ILU0Preconditioner)
    try:
        assert P.ncolors == n
        assert np.array_equal(P.colors(), col.color)
        assert np.array_equal(P.permutation(), col.c + 1)
        cp, rv, nz = P.reordered_matrix()
        wcp, wrv, wnz = color_model.reorder(arrays, col.c)
        assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv) and np.array_equal(bits(nz), bits(wnz))
    finally:
        P.close()


# ---- nested dissection: lu_order -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lu_model(tmp_path_factory):
    return lu_modellib.Model(tmp_path_factory.mktemp("sort_driver_lu"))


def _grid(esp, nx, ny):
    S = lu_modellib.dominant(lu_modellib.edges_pattern(nx * ny, lu_modellib.grid_edges(nx, ny)))
    return from_scipy(esp, S)


def _nd_bits(n, level):
    """lu_order's key: nb = ceil(log2 n) bits of the node's root below db = ceil(log2 rounds) bits of the depth (at least 1 each)"""
    rounds = int(level.max()) + 1
    return max(1, math.ceil(math.log2(n))) + max(1, math.ceil(math.log2(rounds)))


def test_nested_dissection_pass_parity(esp, lu_model):
    """a 10 x 10 grid with leaves of 128 (one round: 7 + 1 bits, one pass) and a 20 x 15 grid with leaves of 8 (9 + 2 or more
    bits: two passes): the permutation, the tree and B against the model"""
    nbits = []
    for nx, ny, leaf in ((10, 10, 128), (20, 15, 8)):
        A = _grid(esp, nx, ny)
        n = nx * ny
        arrays = host_arrays(A)
        want = lu_model.lu(arrays, leaf, 48)
        c, level = esp.nested_dissection(A, leaf, 48)
        assert np.array_equal(c, want.c + 1) and np.array_equal(level, want.level)
        nbits.append(_nd_bits(n, level))
        P = esp.LUFactorization(A, leaf, 48)
        try:
            assert np.array_equal(P.permutation(), want.c + 1)
            lv, root = P.tree()
            assert lv.dtype == np.int32 and np.array_equal(lv, want.level) and np.array_equal(root, want.node_root + 1)
            cp, rv, nz = P.fill_matrix()
            wcp, wrv, wnz = want.B
            assert np.array_equal(cp, wcp) and np.array_equal(rv, wrv) and np.array_equal(bits(nz), bits(wnz))
            v = np.random.default_rng(47).standard_normal(n)
            assert same_bits(P.ldiv(v), want.ldiv(v))
        finally:
            P.close()
    print("nested dissection: key bits", nbits)
    assert passes(nbits[0]) != passes(nbits[1]) and (passes(nbits[0]) + passes(nbits[1])) % 2 == 1


# ---- the tail behind a producer batch: flush_pre_tail ---------------------------------------------------------------------------------
def test_tail_behind_a_producer_batch(esp, orc):
    """The stencil generator's bucket-ordered batch of a 48^3 grid, then 3000 host-appended entries in shuffled column order: no
    pre-sorted stream, so the run-based partition refuses the tail and flush_pre_tail orders it by 8-bit passes on the plan's
    prefix bits, the last of which must land in the buffer the bucket kernel reads (esp_debug_last_partition 5: batch + tail;
    esp_debug_last_run_order 0: ordered by the passes).  A producer partitions only with a prefix of 9 .. 20 bits (prepart_begin,
    csrc/produce.hip), and 17 bits need 4 10^8 entries: two passes are the case there is; the flush is repeated over the stored
    pattern."""
    g = 48
    N = g ** 3
    rng = np.random.default_rng(49)
    A = esp.ExtendableSparseMatrix(N, N)
    O = orc.ExtendableSparseMatrix(N, N)
    for step, seed in enumerate((31, 32)):
        I, J, V = orc.fdrand_stream(g, g, g, rand_mode=1, seed=seed)
        A.generate_fdrand(g, g, g, seed=seed, rand_mode=1)
        O.apply(np.full(len(I), UPDATE, np.uint8), I, J, V)
        k = 3000
        kn = rng.choice(np.array([SET, UPDATE, RAWUPDATE], np.uint8), k)
        In, Jn, Vn = rng.integers(1, N + 1, k), rng.integers(1, N + 1, k), rng.standard_normal(k)
        In[:2], Jn[:2] = (1, N), (1, N)
        A.append(0, In, Jn, Vn, kinds=kn)
        O.apply(kn, In, Jn, Vn)
        A.flush()
        O.flush()
        print("step", step, "last_partition", A.debug_last_partition(), "last_run_order", A.debug_last_run_order())
        if step == 0:
            assert (A.debug_last_partition(), A.debug_last_run_order()) == (5, 0)
        assert_csc_equal(A.sparse().arrays(), O.arrays(), "step %d" % step)


# ---- the readouts: host array and device array agree ----------------------------------------------------------------------------------
def _both(lib, call, p, count, dtype, *lead):
    """call(p, *lead, pointer, on_device) into a NumPy array and into a CUDA tensor"""
    import torch
    host = np.full(count, -7, dtype)
    assert call(p, *lead, host.ctypes.data_as(C.c_void_p), 0) == 0
    dev = torch.full((count,), -7, dtype={np.int64: torch.int64, np.int32: torch.int32, np.float64: torch.float64}[dtype], device="cuda")
    torch.cuda.synchronize()
    assert call(p, *lead, C.c_void_p(dev.data_ptr()), 1) == 0
    got = dev.cpu().numpy()
    assert np.array_equal(host.view(np.uint8), got.view(np.uint8))
    return host


def test_readouts_host_and_device(esp):
    A = esp.fdrand(9, 7, 3)
    n = A.n
    lib = A._d.lib
    P = esp.ColoredPreconditioner(A, esp.ILUAMPreconditioner)
    try:
        assert np.array_equal(_both(lib, lib.esp_precon_colored_colors, P._p, n, np.int64), P.colors())
        assert np.array_equal(_both(lib, lib.esp_precon_colored_perm, P._p, n, np.int64) + 1, P.permutation())
        assert same_bits(_both(lib, lib.esp_precon_get_factor, P._p, len(P.factor()), np.float64), P.factor())
    finally:
        P.close()
    P = esp.LUFactorization(A, 8, 48)
    try:
        assert np.array_equal(_both(lib, lib.esp_precon_lu_perm, P._p, n, np.int64) + 1, P.permutation())
        level, root = P.tree()
        import torch
        hl, hr = np.full(n, -7, np.int32), np.full(n, -7, np.int64)
        assert lib.esp_precon_lu_tree(P._p, hl.ctypes.data_as(C.c_void_p), hr.ctypes.data_as(C.c_void_p), 0) == 0
        dl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        dr = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert lib.esp_precon_lu_tree(P._p, C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr()), 1) == 0
        assert np.array_equal(hl, level) and np.array_equal(hr + 1, root)
        assert np.array_equal(dl.cpu().numpy(), hl) and np.array_equal(dr.cpu().numpy(), hr)
        assert same_bits(_both(lib, lib.esp_precon_get_factor, P._p, len(P.factor()), np.float64), P.factor())
    finally:
        P.close()
    P = esp.ILUKPreconditioner(A, 2)
    try:
        lev = P.fill_levels()
        assert len(lev) == P.stats()["nnz"] and np.array_equal(_both(lib, lib.esp_precon_iluk_levels, P._p, len(lev), np.int32), lev)
    finally:
        P.close()
    # esp_graph_coloring and esp_nested_dissection, which read out of buffers of their own
    import torch
    nc = C.c_int64()
    hc, dc = np.full(n, -7, np.int64), torch.full((n,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.esp_graph_coloring(A._d.h, C.byref(nc), hc.ctypes.data_as(C.c_void_p), 0) == 0
    assert lib.esp_graph_coloring(A._d.h, C.byref(nc), C.c_void_p(dc.data_ptr()), 1) == 0
    assert hc.min() == 0 and hc.max() == nc.value - 1 and np.array_equal(dc.cpu().numpy(), hc)
    c, level = esp.nested_dissection(A, 8, 48)
    dcc, dlv = torch.full((n,), -7, dtype=torch.int64, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.esp_nested_dissection(A._d.h, 8, 48, C.c_void_p(dcc.data_ptr()), C.c_void_p(dlv.data_ptr()), 1) == 0
    assert np.array_equal(dcc.cpu().numpy() + 1, c) and np.array_equal(dlv.cpu().numpy(), level)
