"""The PAIR form of the small bucket kernel (csrc/local_w.hip, pair_k): one workgroup takes two neighbouring producer buckets.

Every flush is compared bit for bit with the same flush pinned to one bucket per workgroup (esp_debug_force_path 42: local_k's small
variant), and the kernel that ran is asserted (esp_debug_last_bucket_pairs)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_PAIRS = 42


def _bits(arrs):
    return [np.ascontiguousarray(x).view(np.uint8).copy() for x in arrs]


def _assert_same(got, want, what):
    assert len(got) == len(want) == 3, what
    for g, w, nm in zip(_bits(got), _bits(want), ("colptr", "rowval", "nzval")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, nm)


def _fdrand(esp, n, force, seed=0x5EED0002, kind=None):
    A = esp.ExtendableSparseMatrix(n ** 3, n ** 3)
    A.debug_force_path(force)
    if kind is None:
        A.generate_fdrand(n, n, n, seed=seed, rand_mode=1)
    else:
        A.generate_fdrand(n, n, n, seed=seed, rand_mode=1, kind=kind)
    A.flush()
    return A


@pytest.mark.parametrize("n", [8, 21, 26, 27, 44, 64])
def test_pairs_small_grids(esp, n):
    """Small cubes: 21^3, 26^3, 27^3 and 44^3 cut into an ODD number of 256-column buckets (the last pair holds one), 8^3 into
    two; against one bucket per workgroup, with UPDATE and RAWUPDATE streams (4-byte keys 2 / 1)."""
    for kind in (None, esp.ESP_RAWUPDATE):
        A = _fdrand(esp, n, 0, kind=kind)
        B = _fdrand(esp, n, NO_PAIRS, kind=kind)
        assert A.debug_last_key_bytes() == 4 and B.debug_last_key_bytes() == 4
        assert A.debug_last_bucket_pairs() == 1, (n, kind)
        assert B.debug_last_bucket_pairs() == 0
        assert A.debug_last_local_small() == 1 and B.debug_last_local_small() == 1
        _assert_same(A.arrays(), B.arrays(), "fdrand %d kind %s" % (n, kind))


def test_pairs_headline_size(esp):
    """256^3: 32 768 pairs of two full buckets -- 512 columns x 12 updates, exactly 6144 entries (the kernel's capacity) in every
    interior pair; the same CSC as one bucket per workgroup, and again on the same handle after reset!."""
    n = 256
    A = _fdrand(esp, n, 0)
    assert A.debug_last_bucket_pairs() == 1
    B = _fdrand(esp, n, NO_PAIRS)
    assert B.debug_last_bucket_pairs() == 0
    want = B.arrays()
    _assert_same(A.arrays(), want, "256^3")
    del B
    A.reset()
    A.generate_fdrand(n, n, n, seed=0x5EED0002, rand_mode=1)
    A.flush()
    assert A.debug_last_bucket_pairs() == 1
    _assert_same(A.arrays(), want, "256^3 after reset!")


def _banded(n, far, seed):
    """12 updates per column (6 rows x 2), in column order: rows near the diagonal, and for `far` columns one row n/2 away"""
    rng = np.random.default_rng(seed)
    J = np.repeat(np.arange(1, n + 1, dtype=np.int64), 12)
    off = np.tile(np.array([-2, -1, 0, 1, 2, 3] * 2, np.int64), n)
    I = np.clip(J + off, 1, n)
    if far:
        cols = rng.choice(n, far, replace=False)
        I[cols * 12 + 5] = (cols + n // 2) % n + 1
    V = rng.standard_normal(len(I))
    V[rng.random(len(I)) < 0.05] = 0.0
    return I, J, V


def _appended(esp, n, I, J, V, force):
    A = esp.ExtendableSparseMatrix(n, n)
    A.debug_force_path(force)
    A.append(esp.ESP_UPDATE, I, J, V)
    A.flush()
    return A


def test_pairs_row_span_falls_back(esp):
    """Caller triplets (4-byte keys, direct colptr): near-diagonal rows take the pair kernel; a stream with rows n/2 away in some
    columns spans more than 2^19 rows inside a pair -- the kernel refuses it, the flush runs again with local_k (the same bits as
    the pinned path) and the handle keeps local_k."""
    n = 1 << 21
    I, J, V = _banded(n, 0, 1)
    A = _appended(esp, n, I, J, V, 0)
    assert A.debug_last_key_bytes() == 4 and A.debug_last_local_small() == 1
    assert A.debug_last_bucket_pairs() == 1
    _assert_same(A.arrays(), _appended(esp, n, I, J, V, NO_PAIRS).arrays(), "banded")
    I2, J2, V2 = _banded(n, 40, 2)
    B = _appended(esp, n, I2, J2, V2, 0)
    assert B.debug_last_bucket_pairs() == 0 and B.debug_last_local_small() == 1
    _assert_same(B.arrays(), _appended(esp, n, I2, J2, V2, NO_PAIRS).arrays(), "far rows")
    B.reset()
    B.append(esp.ESP_UPDATE, I, J, V)
    B.flush()
    assert B.debug_last_bucket_pairs() == 0      # (the handle met a pair the kernel refused)
    _assert_same(B.arrays(), A.arrays(), "after the fall-back")


def test_pairs_two_handles_side_by_side(esp):
    """Two host threads, one handle each, flushing together (a 44^3 stencil with an odd bucket count and a 64^3 one): every
    round bit for bit the pinned one-bucket result."""
    works = [(44, 5), (64, 6)]
    want = [_fdrand(esp, n, NO_PAIRS, seed=s).arrays() for n, s in works]
    bar = threading.Barrier(len(works))
    errors = []

    def run(q):
        try:
            n, s = works[q]
            A = esp.ExtendableSparseMatrix(n ** 3, n ** 3)
            for rnd in range(20):
                A.reset()
                A.generate_fdrand(n, n, n, seed=s, rand_mode=1)
                bar.wait(timeout=300)
                A.flush()
                assert A.debug_last_bucket_pairs() == 1
                _assert_same(A.arrays(), want[q], "handle %d round %d" % (q, rnd))
        except BaseException as ex:  # noqa: BLE001 (reported by the main thread)
            errors.append((q, repr(ex)[:400]))
            bar.abort()

    th = [threading.Thread(target=run, args=(q,)) for q in range(len(works))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
