"""The stencil producer fused into the predicted pair kernel (csrc/local_x.hip, pair_gen_pred_k; esp_handle::LazyStencil): a
full-range fdrand! batch that repeats the handle's last plan on a fresh matrix is not written -- the flush's bucket kernel forms
every column's updates itself, in the pull order tests/stencil_pull.py states and tests/test_stencil_pull.py checks against the
oracle's stream -- and whoever else needs the entries gets the held-back PART launch first (lazy_expand).

Every flush is compared bit for bit (colptr / rowval / nzval) with the same calls on a handle pinned to esp_debug_force_path 44
(the batch is always written: the parent's path), the small grids with the CPU oracle as well, and what happened is asserted
(esp_debug_last_lazy_stencil: 0 not armed, 1 the fused kernel served the flush, 2 armed, then written after all): 1 exactly
where the pinned handle reports a served prediction with the pair kernel and a reused plan."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same

pytestmark = pytest.mark.gpu

NO_LAZY = 44
SEED_A, SEED_B = 0x5EED0002, 0x5EED0B0B

# cubes cannot see swapped hx / hy / hz: 96x40x24 beside them; nz = 1; the "> 2" rules of the boundary terms; nx = 1 (the slow
# node arithmetic); every node on an x boundary; a pair of buckets inside one grid line; one dimension
MUST_SERVE = [(44, 44, 44), (64, 64, 64), (96, 40, 24)]
# A one-dimensional grid holds 4 updates per column: the plan fills a bucket of 4096 to between 45 and 90 %, which makes it 460 to
# 920 columns wide -- 2^9 or 2^10 -- whatever the size, and the small variant of the bucket kernel (and with it the pair form and
# its predicted form, on the pinned handle as well) takes buckets of at most 2^8 columns.  No larger grid of the class is served
# either; the grid stays in the list with the rule asserted (state 0 on every flush) and the results compared.
NOT_PAIRED = [(90000, 1, 1)]
GRIDS = MUST_SERVE + [(300, 300, 1), (512, 2, 96), (96, 512, 2), (1, 300, 300), (2, 220, 220), (1100, 9, 9), (90000, 1, 1)]


def _matrix(esp, N, force):
    A = esp.ExtendableSparseMatrix(N, N)
    A.debug_force_path(force)
    return A


def _what(A):
    return (A.debug_last_predicted(), A.debug_last_bucket_pairs(), A.debug_last_plan_reused())


def _assemble(A, grid, seed, mode=1, kind=None):
    A.reset()
    A.generate_fdrand(*grid, seed=seed, rand_mode=mode, **({} if kind is None else {"kind": kind}))
    A.flush()
    return _what(A), A.debug_last_lazy_stencil()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%dx%d" % g)
def test_fused_equals_written(esp, orc, grid):
    """kinds UPDATE / RAWUPDATE / COO, rand_mode 0 / 1 / 2, seeds A, A, B on one handle per kind (the plan depends on none of
    mode and seed: everything behind the first flush repeats it)"""
    nx, ny, nz = grid
    N = nx * ny * nz
    served = 0
    for kind in (ps.UPDATE, ps.RAWUPDATE, ps.COO):
        A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
        for mode in (0, 1, 2):
            for i, seed in enumerate((SEED_A, SEED_A, SEED_B)):
                what, lazy = _assemble(A, grid, seed, mode, kind)
                bwhat, blazy = _assemble(B, grid, seed, mode, kind)
                print("grid", grid, "kind", kind, "mode", mode, "flush", i + 1, "auto", what, lazy, "pinned", bwhat, blazy)
                assert blazy == 0, (kind, mode, i)
                assert what == bwhat, (kind, mode, i)
                assert lazy == (1 if bwhat == (1, 1, 1) else 0), (kind, mode, i, bwhat)
                got = A.arrays()
                _assert_same(got, B.arrays(), "fdrand %s kind %d mode %d flush %d" % (grid, kind, mode, i + 1))
                if i == 2 and N <= 100000:  # (the small grids: the flush of seed B against the oracle)
                    I, J, V = orc.fdrand_stream(nx, ny, nz, rand_mode=mode, seed=seed)
                    _assert_same(got, ps.oracle_csc(orc, N, N, kind, I, J, V), "oracle %s kind %d mode %d" % (grid, kind, mode))
                if kind != ps.COO:
                    served += lazy
                if grid in MUST_SERVE and kind != ps.COO:
                    assert lazy == (0 if (mode == 0 and i == 0) else 1), (kind, mode, i)
    # every class of grid keeps a served member: the listed one is served (UPDATE and RAWUPDATE, all but the first flush) -- but
    # the one-dimensional grid, which the parent's pair form takes at no size (NOT_PAIRED)
    assert served == (0 if grid in NOT_PAIRED else 2 * 8), served


def _served_then_armed(esp, n=44, seed=SEED_B):
    """an automatic and a pinned handle after a served flush, an armed generator call on each (nothing flushed yet); the armed
    call has another seed than the batch the handle wrote last: what a missing expansion would leave in the buffer is not it"""
    g = (n, n, n)
    A, B = _matrix(esp, n ** 3, 0), _matrix(esp, n ** 3, NO_LAZY)
    for X in (A, B):
        _assemble(X, g, SEED_A)
        _assemble(X, g, SEED_A)
    assert A.debug_last_lazy_stencil() == 1 and B.debug_last_lazy_stencil() == 0
    for X in (A, B):
        X.reset()
        X.generate_fdrand(*g, seed=seed, rand_mode=1)
    assert A.debug_last_lazy_stencil() == 0
    return A, B, g


def _finish(A, B, what, allowed=(0, 2)):
    for X in (A, B):
        X.flush()
    assert A.debug_last_lazy_stencil() in allowed, (what, A.debug_last_lazy_stencil())
    _assert_same(A.arrays(), B.arrays(), what)


def test_expand_append_behind(esp):
    A, B, g = _served_then_armed(esp)
    N = g[0] ** 3
    for X in (A, B):
        X.append(esp.ESP_UPDATE, np.array([1, 5, N], np.int64), np.array([N, 7, 1], np.int64), np.array([1.5, -2.0, 3.0]))
    assert A.debug_last_lazy_stencil() == 2
    _finish(A, B, "append behind the batch")


def test_expand_pending_getindex(esp):
    A, B, g = _served_then_armed(esp)
    n = g[0]
    for i, j in ((1, 1), (2, 1), (n * n + 5, 5), (7, 7 + n), (3, 900)):
        got = []
        for X in (A, B):
            val, found = C.c_double(), C.c_int32()
            X._d.ck(X._d.lib.esp_pending_getindex(X._d.h, i, j, C.byref(val), C.byref(found)))
            got.append((np.float64(val.value).view(np.uint64), found.value))
        assert got[0] == got[1], (i, j, got)
    assert A.debug_last_lazy_stencil() == 2
    _finish(A, B, "getindex on the pending buffer")


def test_pending_count(esp):
    """pending() is the count alone: E entries to every observer, nothing is written for it -- and the flush is still served"""
    A, B, g = _served_then_armed(esp)
    n = g[0]
    assert A._d.pending() == B._d.pending() == 12 * n * n * (n - 1) + 6 * n * n
    assert A.debug_last_lazy_stencil() == 0
    _finish(A, B, "pending()", allowed=(1,))


def test_expand_shard_export(esp):
    import torch
    A, B, g = _served_then_armed(esp)
    n = g[0]
    E = 12 * n * n * (n - 1) + 6 * n * n
    out = []
    for X in (A, B):
        keys = torch.empty(E, dtype=torch.int64, device="cuda")
        vals = torch.empty(E, dtype=torch.float64, device="cuda")
        offs = (C.c_int64 * 2)()
        X._d.ck(X._d.lib.esp_shard_export(X._d.h, 1, C.c_void_p(keys.data_ptr()), C.c_void_p(vals.data_ptr()), offs))
        torch.cuda.synchronize()
        out.append((keys.cpu().numpy(), vals.cpu().numpy().view(np.uint64), list(offs)))
    assert A.debug_last_lazy_stencil() == 2
    assert out[0][2] == out[1][2] == [0, E]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_expand_second_generator_call(esp):
    A, B, g = _served_then_armed(esp)
    for X in (A, B):
        X.generate_fdrand(*g, seed=SEED_B, rand_mode=2)
    assert A.debug_last_lazy_stencil() in (0, 2)
    _finish(A, B, "a second generator call")


def test_over_a_stored_pattern(esp):
    """zero_values + generate + flush: the matrix holds entries, the batch is written in the generator call"""
    g = (44, 44, 44)
    A, B = _matrix(esp, 44 ** 3, 0), _matrix(esp, 44 ** 3, NO_LAZY)
    for X in (A, B):
        _assemble(X, g, SEED_A)
        _assemble(X, g, SEED_A)
        X.zero_values()
        X.generate_fdrand(*g, seed=SEED_B, rand_mode=1)
    _finish(A, B, "over the stored pattern", allowed=(0,))


def test_expand_release_buffers(esp):
    A, B, g = _served_then_armed(esp)
    for X in (A, B):
        X._d.ck(X._d.lib.esp_release_buffers(X._d.h))
        assert X._d.pending() == 0
        X.generate_fdrand(*g, seed=SEED_B, rand_mode=1)
    _finish(A, B, "released buffers", allowed=(0,))
    for X in (A, B):
        _assemble(X, g, SEED_B)
    assert A.debug_last_lazy_stencil() == 1
    _assert_same(A.arrays(), B.arrays(), "served again")


def test_reset_then_another_grid(esp):
    A, B, g = _served_then_armed(esp)
    n = g[0]
    for X in (A, B):
        X.reset()
        X.generate_fdrand(n * n, n, 1, seed=SEED_A, rand_mode=1)
    _finish(A, B, "another grid with the same node count", allowed=(0,))


def test_clone_of_an_armed_batch(esp):
    A, B, g = _served_then_armed(esp)
    Ac, Bc = A.copy(), B.copy()
    assert A.debug_last_lazy_stencil() == 2
    _finish(Ac, Bc, "the clones")
    _finish(A, B, "the originals")


def test_spoiled_table(esp):
    """one entry of the kept table spoiled: the fused kernel misses, the batch is written, the look-back form serves the flush and
    records anew; the next flush is served by the fused kernel again"""
    g = (44, 44, 44)
    A, B = _matrix(esp, 44 ** 3, 0), _matrix(esp, 44 ** 3, NO_LAZY)
    for X in (A, B):
        _assemble(X, g, SEED_A)
        _assemble(X, g, SEED_A)
    A.debug_spoil_predicted()
    what, lazy = _assemble(A, g, SEED_B)
    _assemble(B, g, SEED_B)
    assert (what[0], lazy) == (2, 2) and what[1:] == (1, 1), (what, lazy)
    _assert_same(A.arrays(), B.arrays(), "spoiled table")
    what, lazy = _assemble(A, g, SEED_B)
    assert (what, lazy) == ((1, 1, 1), 1)
    _assert_same(A.arrays(), B.arrays(), "after the miss")


def test_headline_size(esp):
    """256^3, UPDATE, seeds A, A: flush 2 is served by the fused kernel and has the oracle's digest (fd_256_m1)"""
    pin = None
    with open(__file__.rsplit("/", 1)[0] + "/golden/digests_large.txt") as f:
        for line in f:
            p = line.split()
            if p and p[0] == "fd_256_m1":
                pin = dict(x.split("=") for x in p[1:])
    assert pin is not None
    g = (256, 256, 256)
    A = _matrix(esp, 256 ** 3, 0)
    assert _assemble(A, g, SEED_A) == ((0, 1, 0), 0)
    assert _assemble(A, g, SEED_A) == ((1, 1, 1), 1)
    h = hashlib.sha256()
    arrs = A.arrays()
    for a in arrs:
        h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    assert (h.hexdigest(), len(arrs[1])) == (pin["csc"], int(pin["nnz"]))
