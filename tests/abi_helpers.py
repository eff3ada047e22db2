"""Padded device buffers for the C-ABI layout tests (test_gpu_abi_layout.py,
test_gpu_small_stages.py): a logical rows x width matrix placed at an element
offset `lead` of one flat sentinel-filled allocation with row stride `ld`, so
a test can hand the library a pointer that is not the start of an allocation,
with ld != width, and afterwards see whether anything outside the logical
matrix was written."""
import ctypes

import numpy as np
import torch

DEV = "cuda:0"
SENTINEL = -7.25
TAIL = 5  # sentinel elements after the last row's padding

# name -> (lead, ld - width).  C: contiguous.  A: padded, rows and base stay
# 16-byte aligned (ld - width = 8 elements).  B: base off by one element, so
# neither 16-byte aligned nor (for an even width) an even ld: the scalar gates.
LAYOUTS = {"C": (0, 0), "A": (0, 8), "B": (1, 3)}


def padded(a, ld, lead, sentinel=SENTINEL):
    """(pointer to the logical [0, 0], the whole flat device buffer)."""
    a = np.ascontiguousarray(a)
    rows, width = a.shape
    assert ld >= width and lead >= 0
    flat = np.full(lead + rows * ld + TAIL, sentinel, dtype=a.dtype)
    flat[lead:lead + rows * ld].reshape(rows, ld)[:, :width] = a
    buf = torch.from_numpy(flat).to(DEV)
    return ctypes.c_void_p(buf.data_ptr() + lead * a.itemsize), buf


def lay(a, layout, sentinel=SENTINEL):
    """padded() in one of LAYOUTS; returns (pointer, buffer, ld, lead)."""
    lead, pad = LAYOUTS[layout]
    ld = np.shape(a)[1] + pad
    p, buf = padded(a, ld, lead, sentinel)
    return p, buf, ld, lead


def logical(buf, shape, ld, lead):
    """The logical matrix of a padded buffer, as a host array."""
    rows, width = shape
    flat = buf.cpu().numpy()
    return flat[lead:lead + rows * ld].reshape(rows, ld)[:, :width].copy()


def outside_intact(buf, shape, ld, lead, sentinel=SENTINEL):
    """True when the lead-in, the columns width .. ld-1 of every row and the
    tail still hold the sentinel."""
    rows, width = shape
    flat = buf.cpu().numpy()
    mask = np.ones(flat.shape, dtype=bool)
    mask[lead:lead + rows * ld].reshape(rows, ld)[:, :width] = False
    return bool(np.all(flat[mask] == flat.dtype.type(sentinel)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
