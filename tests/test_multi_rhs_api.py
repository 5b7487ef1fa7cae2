"""CPU: many_layout, the layout decision of every call that takes several right-hand sides (A.mul(X), F.ldiv(V), A.solve(B)):
which (n, k) arrays are used in place, which are copied to column-major once, the (ld, k) it reports and what it refuses.
No device is touched."""
import numpy as np
import pytest


def colmajor(holder, ld, n, k):
    """the n x k values a column-major reader with leading dimension ld sees behind holder's first element"""
    if n * k == 0:
        return np.empty((n, k))
    flat = np.lib.stride_tricks.as_strided(holder, ((k - 1) * ld + n,), (8,))
    return np.array([[flat[r * ld + i] for r in range(k)] for i in range(n)])


@pytest.fixture(scope="module")
def layout(esp):
    return esp.many_layout


def test_f_order_is_used_in_place(layout):
    X = np.asfortranarray(np.arange(15.0).reshape(5, 3))
    holder, ld, k = layout(5, X)
    assert holder is X and (ld, k) == (5, 3)


def test_c_order_is_copied_once_to_column_major(layout):
    X = np.arange(15.0).reshape(5, 3)
    holder, ld, k = layout(5, X)
    assert holder is not X and holder.flags.f_contiguous and (ld, k) == (5, 3)
    assert np.array_equal(holder, X) and np.array_equal(colmajor(holder, ld, 5, 3), X)


def test_row_slice_of_f_order_keeps_its_leading_dimension(layout):
    big = np.asfortranarray(np.arange(32.0).reshape(8, 4))
    X = big[1:6]                                          # 5 rows of 8: columns contiguous, ld = 8
    holder, ld, k = layout(5, X)
    assert holder is X and (ld, k) == (8, 4)
    assert np.array_equal(colmajor(holder, ld, 5, 4), X)


def test_other_slices_are_copied(layout):
    big = np.asfortranarray(np.arange(40.0).reshape(10, 4))
    for X in (big[::2], big[:5, ::-1], big.T[:, :5].T[::-1], np.arange(40.0).reshape(5, 8)[:, ::2]):
        holder, ld, k = layout(5, X)
        assert holder is not X and holder.flags.f_contiguous and (ld, k) == (5, X.shape[1])
        assert np.array_equal(colmajor(holder, ld, 5, k), X)
    cols = big[:, 1:3]                                    # a column slice of F-order is F-order itself
    holder, ld, k = layout(10, cols)
    assert holder is cols and (ld, k) == (10, 2)


def test_one_column_one_row_and_empty(layout):
    X = np.asfortranarray(np.arange(24.0).reshape(8, 3))[2:6, 1:2]   # one column: its column stride is never used, ld = n
    holder, ld, k = layout(4, X)
    assert holder is X and (ld, k) == (4, 1)
    Xc = np.arange(12.0).reshape(4, 3)[:, 1:2]            # one column of a C-ordered array: its rows are not contiguous
    holder, ld, k = layout(4, Xc)
    assert holder is not Xc and (ld, k) == (4, 1) and np.array_equal(holder, Xc)
    row = np.arange(6.0).reshape(1, 6)                    # n = 1: the row stride is free, ld is the column stride
    holder, ld, k = layout(1, row)
    assert holder is row and (ld, k) == (1, 6)
    row2 = np.arange(12.0).reshape(2, 6)[1:]
    holder, ld, k = layout(1, row2)
    assert (ld, k) == (1, 6) and np.array_equal(colmajor(holder, ld, 1, 6), row2)
    for shape in ((0, 3), (4, 0), (0, 0)):
        holder, ld, k = layout(shape[0], np.empty(shape))
        assert (ld, k) == (max(shape[0], 1), shape[1]) and holder.shape == shape


def test_refusals(layout):
    for bad in (np.zeros((5, 3, 2)), np.zeros((4, 3)), np.zeros((6, 3)), np.zeros((5, 3), np.float32), np.zeros((5, 3), np.int64),
                np.zeros(5), [[1.0, 2.0]] * 5):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            layout(5, bad)
