"""The structure kept across repeated stencil steps (csrc/local_x.hip, pair_gen_pred_k<.., KEEP>; esp_handle::KeptStructure;
flush_local's fused branch): a fused flush that finds colptr and rowval as the handle's last fused flush of the same plan, table,
grid and kind left them -- and that flush emitted the grid's whole structural pattern -- stores the values alone.

Every flush is compared by the raw bytes of colptr / rowval / nzval with the same calls on a handle pinned to
esp_debug_force_path 45 (the fused kernel's storing form) and with the CPU oracle (every grid is below 10^5 nodes), and
esp_debug_last_kept_structure is asserted: 0 on the first served fused flush, 1 from the next one on, 0 again behind whatever may
have written or moved colptr / rowval, 2 behind a spoiled offset table.

A grid the device does not serve by the fused form is named in a warning (it cannot show the kept form); at least four of the six
must reach state 1."""
import warnings

import numpy as np
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same

pytestmark = pytest.mark.gpu

NO_KEEP = 45
SEEDS = (0x5EED0002, 0x5EED0B0B, 0x5EED0C0C, 0x5EED0D0D)
GRIDS = [(96, 40, 24), (512, 2, 96), (44, 44, 44), (20, 50, 90), (65, 36, 36), (8, 8, 1400)]
G44 = (44, 44, 44)
GA, GB = (20, 50, 90), (50, 20, 90)   # two grids with the same N and the same structural count

_streams = {}   # (grid, mode, seed) -> the oracle's update stream, computed once and never changed
_kept = {}      # grid -> flushes that reached state 1 (test_at_least_four_grids_are_kept reads what test_kept_equals_stored counted)


def _gid(g):
    return "%dx%dx%d" % g


def _structural(grid):
    nx, ny, nz = grid
    return nx * ny * nz + 2 * ((nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1))


def _oracle(orc, grid, mode, seed, kind):
    key = (grid, mode, seed)
    if key not in _streams:
        _streams[key] = orc.fdrand_stream(*grid, rand_mode=mode, seed=seed)
    I, J, V = _streams[key]
    N = grid[0] * grid[1] * grid[2]
    return ps.oracle_csc(orc, N, N, kind, I, J, V)


def _matrix(esp, N, force):
    A = esp.ExtendableSparseMatrix(N, N)
    A.debug_force_path(force)
    return A


def _assemble(A, grid, seed, mode=1, kind=ps.UPDATE):
    """reset!, fdrand!, flush!; returns (served by the fused kernel, kept state)"""
    A.reset()
    A.generate_fdrand(*grid, seed=seed, rand_mode=mode, kind=kind)
    A.flush()
    return A.debug_last_lazy_stencil() == 1, A.debug_last_kept_structure()


def _both(orc, A, B, grid, seed, what, mode=1, kind=ps.UPDATE):
    """one assembly on the automatic and on the pinned handle, both against the oracle; returns A's (served, kept state)"""
    served, kept = _assemble(A, grid, seed, mode, kind)
    bserved, bkept = _assemble(B, grid, seed, mode, kind)
    print(what, "grid", grid, "auto", served, kept, "pinned", bserved, bkept)
    assert bkept == 0, (what, "the pinned handle kept")
    assert served == bserved, (what, served, bserved)
    want = _oracle(orc, grid, mode, seed, kind)
    _assert_same(B.arrays(), want, what + ": pinned against the oracle")
    _assert_same(A.arrays(), want, what + ": against the oracle")
    _assert_same(A.arrays(), B.arrays(), what + ": against the pinned handle")
    return served, kept


def _kept_pair(esp, orc, grid=G44, kind=ps.UPDATE):
    """a handle pair on `grid` whose automatic member has just flushed in the kept form (three assemblies)"""
    N = grid[0] * grid[1] * grid[2]
    A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_KEEP)
    for i in range(3):
        served, kept = _both(orc, A, B, grid, SEEDS[i], "set-up %d" % (i + 1), kind=kind)
    assert (served, kept) == (True, 1), "grid %s is not kept on this device: (served, state) = %s" % (_gid(grid), (served, kept))
    return A, B


@pytest.mark.parametrize("grid", GRIDS, ids=_gid)
def test_kept_equals_stored(esp, orc, grid):
    """UPDATE / RAWUPDATE x rand_mode 0 / 1 / 2, four assemblies with four seeds on one handle: state 0 on the first served fused
    flush, 1 from the next one on, every flush equal to the pinned handle's and the oracle's"""
    N = grid[0] * grid[1] * grid[2]
    kept_flushes = 0
    for kind in (ps.UPDATE, ps.RAWUPDATE):
        for mode in (0, 1, 2):
            A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_KEEP)
            served_before = 0
            for i, seed in enumerate(SEEDS):
                what = "%s kind %d mode %d flush %d" % (_gid(grid), kind, mode, i + 1)
                served, kept = _both(orc, A, B, grid, seed, what, mode, kind)
                assert A._d.nnz() == _structural(grid), what
                # (not served: stored everything; the first served flush stores and arms; the served ones behind it keep)
                assert kept == (1 if served and served_before else 0), (what, served, served_before, kept)
                served_before = served_before + 1 if served else 0
                kept_flushes += kept == 1
    _kept[grid] = kept_flushes
    if kept_flushes == 0:
        warnings.warn("grid %s is not served by the fused stencil kernel on this device: the kept form never ran on it" % _gid(grid))


def test_at_least_four_grids_are_kept(esp, orc):
    for grid in GRIDS:
        if grid not in _kept:  # (run by itself: one handle pair per grid is enough to know)
            N = grid[0] * grid[1] * grid[2]
            A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_KEEP)
            _kept[grid] = sum(_both(orc, A, B, grid, seed, "%s flush %d" % (_gid(grid), i + 1))[1] == 1 for i, seed in enumerate(SEEDS))
    print({_gid(g): n for g, n in _kept.items()})
    missing = [_gid(g) for g in GRIDS if _kept[g] == 0]
    for name in missing:
        warnings.warn("grid %s never reached esp_debug_last_kept_structure 1" % name)
    assert len(GRIDS) - len(missing) >= 4, ("grids that never kept", missing)


def test_small_matrix_is_never_kept(esp, orc):
    """n <= 4096: reset! fills colptr at once, so nothing is kept"""
    for grid in ((16, 16, 16), (64, 8, 8)):
        assert grid[0] * grid[1] * grid[2] == 4096
        A, B = _matrix(esp, 4096, 0), _matrix(esp, 4096, NO_KEEP)
        for i, seed in enumerate(SEEDS):
            _, kept = _both(orc, A, B, grid, seed, "%s flush %d" % (_gid(grid), i + 1))
            assert kept == 0, (grid, i, kept)


def _next_is_stored(orc, A, B, grid=G44, kind=ps.UPDATE, what=""):
    """the next assembly stores everything and is exact; the one behind it as well (whatever its state)"""
    _, kept = _both(orc, A, B, grid, SEEDS[3], what + ": next assembly", kind=kind)
    assert kept == 0, (what, kept)
    _both(orc, A, B, grid, SEEDS[0], what + ": the assembly behind it", kind=kind)


def test_dirichlet_editor_drops_the_structure(esp, orc):
    A, B = _kept_pair(esp, orc)
    marker = np.zeros(A.n, np.uint8)
    marker[::97] = 1
    for X in (A, B):
        X.eliminate_dirichlet(marker)
    _assert_same(A.arrays(), B.arrays(), "after eliminate_dirichlet!")
    _next_is_stored(orc, A, B, what="Dirichlet editor")


def test_append_behind_the_batch_drops_the_structure(esp, orc):
    """entries from device arrays behind the armed batch: the flush is not the fused one; and entries over the stored matrix"""
    import torch
    A, B = _kept_pair(esp, orc)
    N = A.n
    I = torch.tensor([1, 5, N, 7, 7], dtype=torch.int64, device="cuda")
    J = torch.tensor([N, 7, 1, 7, 7 + 44], dtype=torch.int64, device="cuda")
    V = torch.tensor([1.5, -2.0, 3.0, 0.25, -8.0], dtype=torch.float64, device="cuda")
    for X in (A, B):  # (behind the batch, one flush)
        X.reset()
        X.generate_fdrand(*G44, seed=SEEDS[1], rand_mode=1)
        X.append_device(esp.ESP_UPDATE, I, J, V)
        X.flush()
    assert A.debug_last_kept_structure() == 0
    _assert_same(A.arrays(), B.arrays(), "entries behind the batch")
    _next_is_stored(orc, A, B, what="append behind the batch")
    A, B = _kept_pair(esp, orc)
    for X in (A, B):  # (behind a kept flush, over the stored matrix)
        X.append_device(esp.ESP_UPDATE, I, J, V)
        X.flush()
    assert A.debug_last_kept_structure() == 0
    _assert_same(A.arrays(), B.arrays(), "entries over the kept matrix")
    _next_is_stored(orc, A, B, what="append over the stored matrix")


def test_set_csc_drops_the_structure(esp, orc):
    """another matrix of the same size and the same number of entries, uploaded into the same buffers"""
    A, B = _kept_pair(esp, orc, GA)
    other = _matrix(esp, A.n, NO_KEEP)
    _assemble(other, GB, SEEDS[0])
    csc = other.sparse()
    assert csc.nnz() == _structural(GA) == _structural(GB)
    for X in (A, B):
        X.cscmatrix = esp.SparseMatrixCSC(csc.m, csc.n, csc.colptr.copy(), csc.rowval.copy(), csc.nzval.copy())
    _assert_same(A.arrays(), other.arrays(), "after esp_set_csc")
    _next_is_stored(orc, A, B, GA, what="esp_set_csc")


def test_release_buffers_drops_the_structure(esp, orc):
    A, B = _kept_pair(esp, orc)
    for X in (A, B):
        X._d.ck(X._d.lib.esp_release_buffers(X._d.h))
    _next_is_stored(orc, A, B, what="esp_release_buffers")


def test_read_of_the_empty_matrix_drops_the_structure(esp, orc):
    """reset!, then a read of the empty matrix: the lazy colptr := 1 is resolved over the kept colptr"""
    A, B = _kept_pair(esp, orc)
    for X in (A, B):
        X.reset()
        colptr, rowval, nzval = X.arrays()
        assert len(rowval) == len(nzval) == 0 and np.array_equal(colptr, np.ones(X.n + 1, np.int64))
    _next_is_stored(orc, A, B, what="read of the empty matrix")


def test_clone_drops_the_structure(esp, orc):
    A, B = _kept_pair(esp, orc)
    C2, D2 = A.copy(), B.copy()
    D2.debug_force_path(NO_KEEP)
    _assert_same(C2.arrays(), A.arrays(), "the clone")
    _next_is_stored(orc, A, B, what="the clone's source")
    _next_is_stored(orc, C2, D2, what="the clone")


def test_spoiled_table_misses_in_the_kept_form(esp, orc):
    A, B = _kept_pair(esp, orc)
    A.debug_spoil_predicted()
    served, kept = _assemble(A, G44, SEEDS[3])  # (the pinned handle's table is whole: it is served, this one is not)
    assert (served, kept) == (False, 2), (served, kept)
    assert A.debug_last_lazy_stencil() == 2 and A.debug_last_predicted() == 2
    assert _assemble(B, G44, SEEDS[3]) == (True, 0)
    want = _oracle(orc, G44, 1, SEEDS[3], ps.UPDATE)
    _assert_same(A.arrays(), want, "spoiled table: against the oracle")
    _assert_same(A.arrays(), B.arrays(), "spoiled table: against the pinned handle")
    _, kept = _both(orc, A, B, G44, SEEDS[0], "behind the miss")
    assert kept == 0, kept


def test_another_grid_with_the_same_n_is_stored(esp, orc):
    A, B = _kept_pair(esp, orc, GA)
    _next_is_stored(orc, A, B, GB, what="20x50x90 then 50x20x90")


def test_the_other_kind_is_stored(esp, orc):
    A, B = _kept_pair(esp, orc, G44, ps.UPDATE)
    _next_is_stored(orc, A, B, G44, ps.RAWUPDATE, what="UPDATE then RAWUPDATE")
    A, B = _kept_pair(esp, orc, G44, ps.RAWUPDATE)
    _next_is_stored(orc, A, B, G44, ps.UPDATE, what="RAWUPDATE then UPDATE")


def test_stale_structure_guard(esp, orc):
    """G1 kept, then G2 != G1 with the same N, then G1 again: every result is the oracle's"""
    A, B = _kept_pair(esp, orc, GA)
    _both(orc, A, B, GB, SEEDS[1], "G2")
    _both(orc, A, B, GA, SEEDS[2], "G1 again")
    _both(orc, A, B, GA, SEEDS[3], "G1 once more")
    _both(orc, A, B, GB, SEEDS[0], "G2 once more")
