"""CPU: tests/device_views.py on NumPy arrays -- the view holds the values, sits where the lead says, an untouched buffer passes,
and a write beside the view is seen and named, on bits (a write of the canary's own value is no change; a NaN with another
payload is)."""
import re

import numpy as np
import pytest

from device_views import CANARY, GUARD, bits_of, frozen, guarded

DTYPES = ["float64", "int64", "int32", "uint8"]
LEADS = [0, 1, 2, 3, 7]
N = 37


def values_of(dtype, n=N):
    rng = np.random.default_rng(5)
    if dtype == "float64":
        v = rng.standard_normal(n)
        if n > 3:
            v[1], v[2], v[3] = np.nan, -0.0, np.inf
        return v
    return rng.integers(0, 200, n).astype(dtype)


def canary_as(dtype):
    """one element holding the canary's bits"""
    return np.array([CANARY[dtype]], "uint64" if dtype == "float64" else dtype).view(dtype)[0]


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_view_holds_the_values_where_the_lead_says(dtype, lead):
    vals = values_of(dtype)
    g = guarded(vals, lead)
    view, check = g
    assert view.dtype == vals.dtype and view.shape == (N,) and view.flags.c_contiguous
    assert np.array_equal(bits_of(view), bits_of(vals))
    assert g.buf.ctypes.data % 256 == 0 and len(g.buf) == GUARD + lead + N + GUARD
    assert view.ctypes.data == g.buf.ctypes.data + (GUARD + lead) * vals.dtype.itemsize
    assert g.align == view.ctypes.data % 16 == (lead * vals.dtype.itemsize) % 16      # (GUARD elements are a multiple of 16 bytes)
    check()
    assert np.shares_memory(view, g.buf)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", [-1, "n", "n+255", "-lead-512", "n+511"])
def test_a_write_beside_the_view_is_seen_and_named(dtype, lead, where):
    g = guarded(values_of(dtype), lead)
    off = {-1: -1, "n": N, "n+255": N + 255, "-lead-512": -lead - GUARD, "n+511": N + GUARD - 1}[where]
    g.check()
    g.buf[GUARD + lead + off] = 1                      # what a kernel's stray store would leave
    with pytest.raises(AssertionError) as ei:
        g.check("stray")
    assert re.search(r"stray: guard element at offset %d of a view of %d %s" % (off, N, dtype), str(ei.value)), str(ei.value)
    g.buf[GUARD + lead + off] = canary_as(dtype)       # the canary's own bits: no change
    g.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_first_changed_offset_is_reported(dtype):
    g = guarded(values_of(dtype), 1)
    g.buf[GUARD + 1 + N + 3] = 1
    g.buf[GUARD + 1 + N + 200] = 1
    with pytest.raises(AssertionError, match=r"offset %d of" % (N + 3)):
        g.check()
    g.buf[GUARD - 4] = 1                               # in front of the view (offset -5): reported before anything behind it
    g.buf[GUARD] = 1                                   # the lead element itself is a canary too (offset -1)
    with pytest.raises(AssertionError, match=r"offset -5 of"):
        g.check()


def test_the_comparison_is_on_bits():
    """float64: another NaN -- the hardware's default one, or the canary with its sign flipped -- is a change; writes inside
    the view are none"""
    g = guarded(values_of("float64"), 1)
    g.view[:] = np.nan
    g.view[0] = canary_as("float64")
    g.check()
    g.buf[GUARD + 1 + N] = np.nan
    with pytest.raises(AssertionError, match=r"offset %d of" % N):
        g.check()
    g.buf[GUARD + 1 + N] = canary_as("float64")
    g.check()
    g.buf.view(np.uint64)[GUARD] ^= np.uint64(1 << 63)
    with pytest.raises(AssertionError, match=r"offset -1 of"):
        g.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single_element_views(dtype, n):
    g = guarded(values_of(dtype, n), 3)
    assert g.view.shape == (n,)
    g.check()
    g.buf[GUARD + 3 + n] = 1
    with pytest.raises(AssertionError, match=r"offset %d of" % n):
        g.check()


def test_shaped_values_are_laid_out_flat():
    """a 2-D array goes in as its C-order elements: the caller reshapes the view"""
    vals = np.arange(12, dtype=np.int64).reshape(4, 3)
    view, check = guarded(vals, 1)
    assert view.shape == (12,) and np.array_equal(view.reshape(4, 3), vals)
    check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen(dtype):
    view, _ = guarded(values_of(dtype), 1)
    f = frozen(view)
    f.check()
    old = view[5].copy()
    view[5] = 77 if old != 77 else 78
    with pytest.raises(AssertionError, match=r"in: input element 5 of %d \(%s\) was written" % (N, dtype)):
        f.check("in")
    view[5] = old
    f.check()
    if dtype == "float64":          # on bits: -0.0 for +0.0 and a NaN of another payload are writes
        view[2] = 0.0
        with pytest.raises(AssertionError, match="element 2"):
            f.check()
        view[2] = -0.0
        view.view(np.uint64)[1] ^= np.uint64(1)
        with pytest.raises(AssertionError, match="element 1"):
            f.check()


def test_unknown_dtype_is_refused():
    with pytest.raises(TypeError):
        guarded(np.zeros(3, np.float32), 0)
