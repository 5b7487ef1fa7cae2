"""The fold, the record writes and the stores of the fused stencil kernel (csrc/local_x.hip, pair_gen_pred_k; csrc/pair.hpp,
pair_store), as NOTES/round21.md left them:

* rand_mode is a template parameter of FdSource, and with kind UPDATE and mode 0 or 1 a row is present exactly when its flag is on
  (no value is zero): the off-diagonal records are -v, the diagonal is summed in call order.  Mode 2 and RAWUPDATE keep the fold.
* every lane writes its present rows to LDS behind the rows' flags (the unpredicated form for a wave whose lanes all hold seven
  rows was measured and dropped; its grids stay: they are the edges of the record writes and of the FLAGS fold);
* pair_store stores two records per lane and round, 16 bytes, behind one 8-byte record where the pair's start is odd and in front
  of one where a record is left over.

Everything must give the bits of path 44 (fdrand_part_k's stream folded by pair_pred_k), as in test_stencil_pair_values_gpu.py:
per grid four assemblies with four seeds, modes 0 / 1 / 2 x UPDATE / RAWUPDATE, an automatic handle against one pinned to path 44
by the raw bytes of colptr / rowval / nzval, grids below 10^5 nodes against the CPU oracle too; the states are (0, 1, 1, 1) and
the kept structure (0, 0, 1, 1): the look-back build, the storing form, the KEEP form twice.

The grids are the smallest at which each part can go wrong AND the fused kernel runs: a repeated fdrand! keeps its plan only when
the partition has more than 8 prefix bits (csrc/produce.hip, prepart_begin), which takes more than 2^16 columns -- 64 x 9 x 9 on an
MI355X: (predicted, pairs, reused) = (0, 1, 0) on every flush, the kernel never runs.  So each grid keeps the x extent its edge
case needs and takes y and z that give 66 000 to 70 000 nodes.  Record writes: every wave holds i = 1 and i = nx (64 x 33 x 33),
one boundary lane per wave (128 x 23 x 23), one of three waves is wholly interior (192 x 19 x 19), 256 x 17 x 16, and ny = 2 /
nz = 2, where the boundary terms are off and no column holds seven rows.  Stores: a last pair of one column (1 x 257 x 257 and
33 x 2017 x 1: 129 x 512 + 1 and 130 x 512 + 1 nodes), and starts and lengths of both parities for every width a pair can have --
checked on the CPU from the oracle's colptr (test_store_grids_cover_both_parities).  One handle assembled on 100 x 100 x 10,
10 x 100 x 100 and 100 x 100 x 10 again: what the kernel takes from the spacings must follow the grid."""
import numpy as np
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same
from test_stencil_share_gpu import NO_LAZY, _both, _matrix

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED0002, 0x5EED0B0B, 0x5EED0C0C, 0x5EED0D0D)

DENSE_GRIDS = [(64, 33, 33), (128, 23, 23), (192, 19, 19), (256, 17, 16), (130, 2, 260), (70, 480, 2)]
STORE_GRIDS = [(1, 257, 257), (33, 2017, 1), (3, 7, 4999), (255, 37, 11)]
ONE_COLUMN_LAST = ((1, 257, 257), (33, 2017, 1))
GRIDS = DENSE_GRIDS + STORE_GRIDS
WIDTHS = (128, 256, 512)  # columns of a pair

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
def test_fold_and_stores_equal_written(esp, orc, grid, kind):
    """rand_mode 0 / 1 / 2, four assemblies with four seeds per handle: the arrays of path 44 on every flush, the storing form on
    the first served flush and the KEEP form behind it"""
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
        assert served == [0, 1, 1, 1], (_gid(grid), mode, served)
        assert kept == [0, 0, 1, 1], (_gid(grid), mode, kept)


def test_store_grids_cover_both_parities(orc):
    """the start and the length of every pair, from the oracle's colptr, for every width a pair can have: both parities of each
    occur among the store grids (an odd start takes the single record in front, an odd rest the one behind)"""
    for width in WIDTHS:
        starts, lengths = set(), set()
        for grid in STORE_GRIDS:
            colptr = np.asarray(orc.fdrand(*grid, rand_mode=1, seed=SEEDS[0], style=orc.KIND_UPDATE).arrays()[0], dtype=np.int64)
            N = grid[0] * grid[1] * grid[2]
            assert colptr.size == N + 1
            edges = np.append(np.arange(0, N, width), N)
            first = colptr[edges] - 1
            starts |= set((first[:-1] & 1).tolist())
            lengths |= set((np.diff(first) & 1).tolist())
            if grid in ONE_COLUMN_LAST:  # (the last pair holds one column: fewer than four records)
                assert edges[-1] - edges[-2] == 1 and first[-1] - first[-2] < 4, (grid, width)
        print("width", width, "start parities", starts, "length parities", lengths)
        assert starts == {0, 1} and lengths == {0, 1}, (width, starts, lengths)


def test_one_handle_three_grids(esp):
    """one handle, N = 100 000, assembled as 100 x 100 x 10, then 10 x 100 x 100, then 100 x 100 x 10 again, three assemblies each:
    every flush equals path 44's -- whatever the kernel keeps of a grid's spacings must not outlive the grid"""
    N = 100000
    A, B = _matrix(esp, N, 0), _matrix(esp, N, NO_LAZY)
    served = []
    for r, grid in enumerate(((100, 100, 10), (10, 100, 100), (100, 100, 10))):
        for i in range(3):
            served.append(_both(A, B, grid, SEEDS[(r + i) % 4], "grid %s assembly %d" % (_gid(grid), i + 1)))
    print("served", served)
    # per grid: the look-back build under the new plan, the storing form, the KEEP form -- the fused kernel runs behind every change
    assert served == [0, 1, 1] * 3, served
