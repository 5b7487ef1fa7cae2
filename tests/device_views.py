"""Caller-owned arrays at odd offsets between guard bands (test infrastructure: no fixtures, no conftest).

Every GPU test used to hand the library a freshly allocated tensor: it starts on the allocator's granule and is followed by slack
nobody looks at.  `guarded(values, lead)` puts the values into the middle of one larger buffer instead --

    | guard canaries | lead canaries | values (the view) | guard canaries |

-- so that the view's address is `lead` elements off an aligned base and every element beside it holds a bit pattern no result can
equal.  `check()` compares those elements bit for bit afterwards; `frozen(view)` does the same for the contents of an input.
Works on NumPy arrays and on CUDA torch tensors alike (the comparisons of a tensor run on its device; only the verdict comes back).
"""
import numpy as np

GUARD = 512   # elements on either side: a 256-element chunk padded past n, plus a stride error of one chunk

# one pattern per element type, none of which a result here can equal: a quiet NaN with a payload no arithmetic produces (the
# hardware's own NaN is 0x7FF8000000000000; payloads of operands are never these bits), odd integers far outside every index range
CANARY = {
    "float64": 0x7FF8DEADBEEF5A5B,
    "int64": 0x5A5BC0DEDEADBEEF,
    "int32": 0x5A5BBEEF,
    "uint8": 0xA5,
}
_BITS = {"float64": "uint64", "int64": "int64", "int32": "int32", "uint8": "uint8"}   # the integer type the bits are compared as


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _name(x):
    """'float64', 'int64', 'int32' or 'uint8' for a NumPy array or a torch tensor"""
    name = str(x.dtype).replace("torch.", "")
    if name not in CANARY:
        raise TypeError("device_views: no canary for dtype %s" % name)
    return name


def _ptr(x):
    return x.data_ptr() if _is_tensor(x) else x.ctypes.data


def _as_bits(x, name):
    """the same memory as integers of the element's width"""
    if _is_tensor(x):
        import torch
        return x.view(torch.int64 if name == "float64" else getattr(torch, _BITS[name]))   # (torch compares no uint64)
    return x.view(_BITS[name])


def _fill(buf, name):
    c = CANARY[name]
    if _is_tensor(buf):
        import torch
        if name == "float64":
            buf.view(torch.int64).fill_(c - (1 << 64) if c >= 1 << 63 else c)
        else:
            buf.fill_(c)
    else:
        _as_bits(buf, name)[...] = np.array(c, _BITS[name])


def _changed(part, name):
    """indices of the elements of `part` that no longer hold the canary's bits (a NumPy int64 array)"""
    c = CANARY[name]
    if _is_tensor(part):
        import torch
        if part.numel() == 0:
            return np.empty(0, np.int64)
        if name == "float64":
            bad = part.view(torch.int64) != (c - (1 << 64) if c >= 1 << 63 else c)
        else:
            bad = part != c
        if not bool(bad.any()):
            return np.empty(0, np.int64)
        return torch.nonzero(bad).reshape(-1).cpu().numpy().astype(np.int64)
    return np.flatnonzero(_as_bits(part, name) != np.array(c, _BITS[name])).astype(np.int64)


class Guarded(tuple):
    """(view, check) with the alignment the view claims: `.align` = view.data_ptr() % 16, `.buf` the whole buffer"""

    def __new__(cls, view, check, align, buf):
        self = super().__new__(cls, (view, check))
        self.view, self.check, self.align, self.buf = view, check, align, buf
        return self


def guarded(values, lead, guard=GUARD):
    """-> (view, check): `values` (1-D, or anything that flattens) copied to offset guard + lead of one flat canary-filled buffer
    of guard + lead + n + guard elements of its dtype, on the device `values` lives on.  view = buf[guard + lead : guard + lead + n];
    check() asserts that every canary on both sides is unchanged bit for bit and names the first changed offset RELATIVE TO THE
    VIEW (-1 the element in front of it, n the first behind it).  The result also carries .align = view address % 16 and .buf."""
    name = _name(values)
    lead, guard = int(lead), int(guard)
    assert lead >= 0 and guard >= 0
    if _is_tensor(values):
        import torch
        flat = values.reshape(-1)
        n = int(flat.numel())
        buf = torch.empty(guard + lead + n + guard, dtype=values.dtype, device=values.device)
        itemsize = buf.element_size()
    else:
        flat = np.ascontiguousarray(values).reshape(-1)
        n = int(flat.size)
        itemsize = flat.dtype.itemsize
        # NumPy promises 16 bytes at most: over-allocate and start on a 256-byte boundary, like the device allocator
        raw = np.empty((guard + lead + n + guard) * itemsize + 256, np.uint8)
        off = (-raw.ctypes.data) % 256
        buf = raw[off:off + (guard + lead + n + guard) * itemsize].view(flat.dtype)
    assert _ptr(buf) % 256 == 0, "device_views: the buffer's base is not 256-byte aligned"
    _fill(buf, name)
    lo = guard + lead
    view = buf[lo:lo + n]
    if n:
        if _is_tensor(values):
            view.copy_(flat)
        else:
            view[...] = flat
    align = (_ptr(buf) + lo * itemsize) % 16          # (an empty view need not report an address of its own)
    assert n == 0 or _ptr(view) == _ptr(buf) + lo * itemsize

    def check(what=""):
        bad = _changed(buf[:lo], name)
        if len(bad) == 0:
            bad = _changed(buf[lo + n:], name)
            first = None if len(bad) == 0 else n + int(bad[0])
        else:
            first = int(bad[0]) - lo
        assert first is None, "%sguard element at offset %d of a view of %d %s elements was written (%d changed on that side)" % (
            what + ": " if what else "", first, n, name, len(bad))

    return Guarded(view, check, align, buf)


class frozen:
    """frozen(view): a snapshot of an input's bits; .check() asserts afterwards that nobody wrote to it (names the first index)"""

    def __init__(self, view):
        self.view, self.name = view, _name(view)
        flat = _as_bits(view.reshape(-1), self.name)
        self.bits = flat.clone() if _is_tensor(view) else flat.copy()

    def check(self, what=""):
        now = _as_bits(self.view.reshape(-1), self.name)
        if _is_tensor(self.view):
            import torch
            bad = now != self.bits
            first = int(torch.nonzero(bad).reshape(-1)[0]) if bool(bad.any()) else None
        else:
            idx = np.flatnonzero(now != self.bits)
            first = int(idx[0]) if len(idx) else None
        assert first is None, "%sinput element %d of %d (%s) was written" % (what + ": " if what else "", first, now.shape[0], self.name)


def bits_of(x):
    """a host copy of the bits of a NumPy array or tensor, as integers (for comparisons across the two)"""
    name = _name(x)
    if _is_tensor(x):
        return _as_bits(x.reshape(-1), name).cpu().numpy().view(_BITS[name])
    return _as_bits(np.ascontiguousarray(x).reshape(-1), name).copy()
