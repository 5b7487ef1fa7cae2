"""The march of the fused stencil kernel (csrc/local_x.hip, pair_gen_pred_k; NOTES/round22.md): a workgroup handles L consecutive
z planes of the same 512 (i, j) columns.  It forms once what does not depend on the plane (the reciprocals, the node's (i, j, k),
the counter, the strides), advances k by 1 and the counter by 6 nx ny GOLDEN per plane, and takes the z pair towards l - nx ny
from the register that formed it one plane below -- a draw in the workgroup's first plane only.  A grid conforms when nx ny is a
multiple of the columns of a pair (2 << cl_bits); every other grid runs one plane per workgroup, as before.

Everything must give the bits of path 44 (fdrand_part_k's stream folded by pair_pred_k), as in test_stencil_fold_store_gpu.py:
per grid four assemblies with four seeds, modes 0 / 1 / 2 x UPDATE / RAWUPDATE, an automatic handle against one pinned to path 44
by the raw bytes of colptr / rowval / nzval, grids below 10^5 nodes against the CPU oracle too; the states are (0, 1, 1, 1), the
kept structure (0, 0, 1, 1) and the march (0, L, L, L): the look-back build, the storing form, the KEEP form twice -- both forms
march.

The fused kernel runs only where the plan is kept (more than 2^16 columns), and the automatic rule gives a grid of that size
L = 1 (it wants 10.75 rounds of the workgroups the device holds), so the march is forced (debug_force_march) and every grid has 66 000 to 131 072
nodes.  nx ny is a multiple of 512 on the conforming grids: they conform whatever width (128, 256, 512) the plan cuts."""
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same
from test_stencil_share_gpu import NO_LAZY, _assemble, _both, _matrix

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED0002, 0x5EED0B0B, 0x5EED0C0C, 0x5EED0D0D)
KINDS = pytest.mark.parametrize("kind", (ps.UPDATE, ps.RAWUPDATE), ids=("update", "rawupdate"))

# one pair per plane at width 512 | odd nz: a tail chunk | | several pairs per plane, a tail chunk of one plane | nz = 2 < L, the
# z boundary rule off | nz = 1 | ny = 2: the y boundary rule off | ny = 1 | nx = 1 | nx = 2
CONFORMING = [(64, 8, 130), (32, 16, 131), (128, 4, 129), (64, 64, 17), (256, 256, 2), (512, 129, 1), (256, 2, 130), (512, 1, 130),
              (1, 512, 130), (2, 256, 130)]
LENGTHS = [((64, 64, 17), L) for L in (2, 3, 17, 64)] + [((64, 8, 130), L) for L in (2, 130)]  # (L = 8: CONFORMING)
NOT_CONFORMING = [(100, 100, 10), (130, 8, 64)]  # nx ny % 128 == 16

_streams = {}  # (grid, mode) -> the oracle's update stream of the last seed, computed once and never changed


def _gid(g):
    return "%dx%dx%d" % g


def _oracle(orc, grid, mode, kind):
    if (grid, mode) not in _streams:
        _streams[(grid, mode)] = orc.fdrand_stream(*grid, rand_mode=mode, seed=SEEDS[-1])
    I, J, V = _streams[(grid, mode)]
    N = grid[0] * grid[1] * grid[2]
    return ps.oracle_csc(orc, N, N, kind, I, J, V)


def _run(esp, orc, grid, kind, force, expect):
    """modes 0 / 1 / 2, four assemblies with four seeds per handle under a forced march: path 44's arrays on every flush, the
    states, and the march `expect(A)` says (asked behind the first flush, when the cut is known)"""
    N = grid[0] * grid[1] * grid[2]
    for mode in (0, 1, 2):
        A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
        A.debug_force_march(force)
        served, kept, march = [], [], []
        for i, seed in enumerate(SEEDS):
            what = "%s L %d kind %d mode %d flush %d" % (_gid(grid), force, kind, mode, i + 1)
            served.append(_both(A, B, grid, seed, what, mode, kind))
            kept.append(A.debug_last_kept_structure())
            march.append(A.debug_last_march())
        L = expect(A)
        print(_gid(grid), "L", force, "kind", kind, "mode", mode, "served", served, "kept", kept, "march", march, "cut", A.debug_last_bucket_cut())
        if N < 100000:  # (the last flush against the oracle)
            _assert_same(A.arrays(), _oracle(orc, grid, mode, kind), "oracle %s kind %d mode %d" % (_gid(grid), kind, mode))
        assert served == [0, 1, 1, 1], (_gid(grid), mode, served)
        assert kept == [0, 0, 1, 1], (_gid(grid), mode, kept)
        assert march == [0, L, L, L], (_gid(grid), mode, march, L)


@KINDS
@pytest.mark.parametrize("grid", CONFORMING, ids=_gid)
def test_march_equals_written(esp, orc, grid, kind):
    """L = 8 forced on the conforming grids; nz below 8 clamps it (256 x 256 x 2: 2; 512 x 129 x 1: 1)"""
    _run(esp, orc, grid, kind, 8, lambda A: min(8, grid[2]))


@KINDS
@pytest.mark.parametrize("grid,L", LENGTHS, ids=lambda v: _gid(v) if isinstance(v, tuple) else "L%d" % v)
def test_march_lengths(esp, orc, grid, L, kind):
    """L = 2, 3, nz and beyond nz (clamped): chunks of every phase against the tail"""
    _run(esp, orc, grid, kind, L, lambda A: min(L, grid[2]))


@KINDS
@pytest.mark.parametrize("grid", NOT_CONFORMING, ids=_gid)
def test_not_conforming_runs_one_plane(esp, orc, grid, kind):
    """nx ny % 128 == 16: whatever the cut, a plane is no whole number of pairs -- one plane per workgroup, served, the same bits"""
    assert (grid[0] * grid[1]) % 128 == 16
    _run(esp, orc, grid, kind, 8, lambda A: 1)


@KINDS
def test_plane_of_256_columns_follows_the_cut(esp, orc, kind):
    """16 x 16 x 260: nx ny = 256 is a whole number of pairs exactly when a pair has at most 256 columns"""
    def expect(A):
        cl_bits, _ = A.debug_last_bucket_cut()
        return 8 if (2 << cl_bits) <= 256 else 1
    _run(esp, orc, (16, 16, 260), kind, 8, expect)


def test_one_handle_three_grids(esp):
    """one handle, N = 66 560, assembled as 64 x 8 x 130, then 130 x 8 x 64 (does not conform), then 64 x 8 x 130 again, three
    assemblies each: every flush equals path 44's, and nothing the march keeps of a grid outlives the grid"""
    N = 64 * 8 * 130
    A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
    A.debug_force_march(8)
    served, march = [], []
    for r, grid in enumerate(((64, 8, 130), (130, 8, 64), (64, 8, 130))):
        for i in range(3):
            served.append(_both(A, B, grid, SEEDS[(r + i) % 4], "grid %s assembly %d" % (_gid(grid), i + 1)))
            march.append(A.debug_last_march())
    print("served", served, "march", march)
    assert served == [0, 1, 1] * 3, served
    assert march == [0, 8, 8, 0, 1, 1, 0, 8, 8], march


def test_spoiled_table_under_the_march(esp):
    """64 x 64 x 17, L = 8: one entry of the kept table spoiled behind two served flushes -- the missing pair stops its workgroup's
    march, the miss arrives through the host word (state 2, the right matrix), and the next two assemblies are served"""
    grid = (64, 64, 17)
    N = 64 * 64 * 17
    A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
    A.debug_force_march(8)
    for i, seed in enumerate((SEEDS[0], SEEDS[1], SEEDS[2])):
        lazy = _both(A, B, grid, seed, "before the miss, assembly %d" % (i + 1))
        assert lazy == (1 if i else 0) and A.debug_last_march() == (8 if i else 0), (i, lazy, A.debug_last_march())
    A.debug_spoil_predicted()
    what, lazy = _assemble(A, grid, SEEDS[3])
    _assemble(B, grid, SEEDS[3])
    assert (what[0], lazy) == (2, 2) and what[1:] == (1, 1), (what, lazy)
    assert A.debug_last_march() == 0
    _assert_same(A.arrays(), B.arrays(), "spoiled table")
    for i, seed in enumerate((SEEDS[3], SEEDS[0])):
        assert _both(A, B, grid, seed, "after the miss, assembly %d" % (i + 1)) == 1
        assert A.debug_last_march() == 8


# the march NOTES/round22.md records as chosen for the flagship grid (256^3, pairs of 512 columns) on an MI355X
FLAGSHIP_MARCH = 3


def test_march_rule(esp):
    """the automatic rule as a pure function: its edges, and the flagship grid on the running device"""
    import torch
    rule = esp.ExtendableSparseMatrix.debug_march_rule
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for grid in NOT_CONFORMING:  # (a plane is no whole number of pairs at any width)
        for cl_bits in (6, 7, 8):
            assert rule(*grid, cl_bits, 1) == 1, (grid, cl_bits)
    assert rule(16, 16, 260, 8, 1) == 1 and rule(16, 16, 260, 7, 1) == 3  # (256 columns a plane: pairs of 512 / of 256)
    assert rule(512, 512, 1, 8, 1) == 1 and rule(512, 512, 2, 8, 1) == 1  # nz = 1, nz below the march
    assert rule(256, 256, 256, 9, 1) == 1 and rule(256, 256, 256, -1, 1) == 1  # (no such pair: more than 512 columns, no cut)
    for nz in range(1, 40):  # one plane or the one measured march, never more than nz
        assert rule(512, 512, nz, 8, 1) in ((1, 3) if nz >= 3 else (1,)), nz
    # 256^3 at width 512: 128 pairs a plane, 128 ceil(256 / 3) = 11 008 workgroups in rounds of 4 per compute unit.  On 256 units
    # that is 10.75 rounds, 33 planes a slot against the 32.25 -> 33 of one plane per workgroup: the measured case.  More rounds
    # (fewer units) march too; 304 units leave 9.05 rounds, 512 and more fewer still: one plane
    assert [rule(256, 256, 256, 8, cu) for cu in (32, 64, 128, 256, 304, 512, 1024)] == [3, 3, 3, 3, 1, 1, 1]
    # (255 planes: 85 chunks, 10.625 rounds -- under the measured 10.75; 128^3 fills the device 4 times with one plane each)
    assert rule(256, 256, 255, 8, 256) == 1 and rule(128, 128, 128, 8, 256) == 1 and rule(512, 512, 512, 8, 256) == 3
    print("compute units", cus, "march of 256^3", rule(256, 256, 256, 8, cus))
    assert rule(256, 256, 256, 8, cus) == FLAGSHIP_MARCH
    for grid in CONFORMING:  # (what the tests force is not what the rule gives: a grid of this size fills no device ten times)
        assert rule(*grid, 8, cus) == 1
