"""The pair values of the fused stencil kernel (csrc/local_x.hip, pair_gen_pred_k; FdSource): a quotient by hx, hy or hz is the
product, the exact remainder and the final fma on a reciprocal each thread forms once (espgen::SharedDiv::quot_mid), and the x and y
pair values of a column's lower neighbours come from the LDS slots of lanes t - 1 and t - nx wherever those lanes belong to the
workgroup, from a draw of their own elsewhere.

Both must give the bits of path 44 -- fdrand_part_k's plain `/` on every pair, folded by pair_pred_k: independent code -- so every
flush of four assemblies (four seeds) on an automatic handle is compared by the raw bytes of colptr / rowval / nzval with the same
calls on a handle pinned to esp_debug_force_path 44, the grids below 10^5 nodes with the CPU oracle as well.  The second assembly
is the first served fused flush (the storing form, which arms the kept structure: n > 4096), the third and the fourth run the KEEP
form; esp_debug_last_lazy_stencil is 1 exactly where the pinned handle reports (predicted, pairs, reused) = (1, 1, 1).

The grids: spacings 1 / n whose mantissas are awkward in all three directions (a reciprocal that is no power of two, so the
quotient's last bit depends on the final fma); nx = 1 (no x pair; the y neighbour is lane t - 1) and ny = 1 (no y pair); a y
neighbour that straddles the pair's first lane and a wave's edge (nx = 96: slots t - 96 cross the 64-lane waves; nx = 200: lanes
below 200 draw, the lanes above read); nx above the pair's width (the y value is never in the workgroup)."""
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same
from test_stencil_share_gpu import NO_LAZY, _both, _matrix

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED0002, 0x5EED0B0B, 0x5EED0C0C, 0x5EED0D0D)

# class -> grids, all below 1.1 10^5 nodes
CLASSES = {
    "awkward mantissas in all three directions": [(255, 37, 11), (257, 19, 21), (100, 100, 10), (3, 7, 4999)],
    "nx = 1": [(1, 300, 300)],
    "ny = 1": [(300, 1, 300)],
    "y neighbour across the pair's first lane and a wave's edge": [(96, 33, 33), (200, 23, 23)],
    "nx above the pair's width": [(600, 13, 13)],
}
GRIDS = [g for gs in CLASSES.values() for g in gs]
# the grids the predicted form serves on its repeated assemblies (what the pinned handle showed on an MI355X)
SERVED = {g: True for g in GRIDS}

_streams = {}  # (grid, mode) -> the oracle's update stream of the last seed, computed once and never changed


def _gid(g):
    return "%dx%dx%d" % g


def _oracle(orc, grid, mode, kind):
    if (grid, mode) not in _streams:
        _streams[(grid, mode)] = orc.fdrand_stream(*grid, rand_mode=mode, seed=SEEDS[-1])
    I, J, V = _streams[(grid, mode)]
    N = grid[0] * grid[1] * grid[2]
    return ps.oracle_csc(orc, N, N, kind, I, J, V)


@pytest.mark.parametrize("kind", (ps.UPDATE, ps.RAWUPDATE), ids=("update", "rawupdate"))
@pytest.mark.parametrize("grid", GRIDS, ids=_gid)
def test_pair_values_equal_written(esp, orc, grid, kind):
    """rand_mode 0 / 1 / 2, four assemblies with four seeds per handle: the same arrays as path 44 on every flush, the rule of the
    state, the storing form on the first served flush and the KEEP form behind it"""
    N = grid[0] * grid[1] * grid[2]
    for mode in (0, 1, 2):
        A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
        served, kept = [], []
        for i, seed in enumerate(SEEDS):
            what = "%s kind %d mode %d flush %d" % (_gid(grid), kind, mode, i + 1)
            served.append(_both(A, B, grid, seed, what, mode, kind))
            kept.append(A.debug_last_kept_structure())
        print(_gid(grid), "kind", kind, "mode", mode, "served", served, "kept", kept)
        if N < 100000:  # (the last flush against the oracle)
            _assert_same(A.arrays(), _oracle(orc, grid, mode, kind), "oracle %s kind %d mode %d" % (_gid(grid), kind, mode))
        if SERVED[grid]:  # the look-back build, the storing form (it arms), the KEEP form twice
            assert served == [0, 1, 1, 1], (_gid(grid), mode, served)
            assert kept == [0, 0, 1, 1], (_gid(grid), mode, kept)
        else:
            assert served == [0, 0, 0, 0] and kept == [0, 0, 0, 0], (_gid(grid), mode, served, kept)


def test_every_class_is_served():
    """every class holds a grid the fused kernel serves (a grid that is not served stays, with state 0 asserted above)"""
    for name, grids in CLASSES.items():
        assert any(SERVED[g] for g in grids), name
