"""CPU: the pull order of the stencil generator (tests/stencil_pull.py) against the oracle's stream, column by column and bit for
bit -- the order the fused pair kernel (csrc/local_x.hip) forms a column's updates in, which test_lazy_stencil_gpu.py relies on."""
import pytest

import stencil_pull as sp

SEED = 0x5EED0002


@pytest.fixture(scope="module")
def columns(orc):
    """(grid, rand_mode) -> (the model's columns, the oracle's), computed once"""
    out = {}
    for nx, ny, nz in sp.GRIDS:
        N = nx * ny * nz
        for mode in (0, 1, 2):
            D = sp.draws(orc.uniform, N, mode, SEED)
            model = [sp.column_pull(l, nx, ny, nz, D) for l in range(1, N + 1)]
            want = sp.stream_by_column(*orc.fdrand_stream(nx, ny, nz, rand_mode=mode, seed=SEED), N)
            out[(nx, ny, nz, mode)] = (model, want)
    return out


def test_pull_order_is_the_streams(columns):
    assert len(columns) == 3 * 11
    for key, (model, want) in columns.items():
        assert len(model) == len(want)
        for l, (m, w) in enumerate(zip(model, want), 1):
            assert sp.bits(m) == sp.bits(w), (key, l)


def test_no_run_above_twelve(columns):
    longest = max(len(m) for model, _ in columns.values() for m in model)
    assert longest == sp.MAX_RUN


def test_rows_strictly_increasing(columns):
    """sorted by (row, call order) a column's rows are its lower neighbours, the diagonal, its upper neighbours: at most seven
    distinct rows, every off-diagonal row holding exactly one update, and the pull order lists the distinct rows of the lower
    pairs and of the upper pairs in increasing order already"""
    for key, (model, _) in columns.items():
        for l, m in enumerate(model, 1):
            rows = [r for r, _ in m]
            off = [r for r in rows if r != l]
            assert len(set(off)) == len(off), (key, l)
            assert len(set(rows)) <= 7, (key, l)
            lower, upper = [r for r in off if r < l], [r for r in off if r > l]
            assert lower == sorted(lower) and upper == sorted(upper), (key, l)
            # and the stable sort by row leaves the diagonal's updates in call order between them
            srt = sp.column_sorted(m)
            assert [r for r, _ in srt] == lower + [l] * (len(rows) - len(off)) + upper, (key, l)
            assert [v for r, v in srt if r == l] == [v for r, v in m if r == l], (key, l)
