"""CPU: the Householder QR entry points (tg_qr_r, tg_qr_r_workspace_size,
tg_u_factor_last_path) are exported, bound, and reject invalid arguments
before any device work (no compute calls -- there is no GPU here)."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "gptq-svd_amd", "libtruncgptq.so")
NAMES = ("tg_qr_r", "tg_qr_r_workspace_size", "tg_u_factor_last_path")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is not built (run build() of __graft_entry__.py first)")
    L = ctypes.CDLL(LIB)
    L.tg_last_error.restype = ctypes.c_char_p
    L.tg_qr_r.restype = ctypes.c_int
    L.tg_qr_r.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    L.tg_qr_r_workspace_size.restype = ctypes.c_size_t
    L.tg_qr_r_workspace_size.argtypes = [ctypes.c_int, ctypes.c_int]
    return L


def test_symbols_exported_and_bound(lib):
    import gptq_svd_amd._lib as B
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in B._SIGS and name in B.EXPORTED, name
    lib.tg_version.restype = ctypes.c_int
    assert lib.tg_version() >= 2
    lib.tg_u_factor_last_path.restype = ctypes.c_int
    assert lib.tg_u_factor_last_path() in (0, 1, 2)


def test_argument_errors_without_gpu(lib):
    p = ctypes.c_void_p(256)
    assert lib.tg_qr_r(None, None, 8, 4, 8, p, 1 << 20) == -2       # null A
    assert b"argument 2" in lib.tg_last_error()
    assert lib.tg_qr_r(None, p, 8, 9, 8, p, 1 << 20) == -4          # k > n
    assert b"argument 4" in lib.tg_last_error()
    assert lib.tg_qr_r(None, p, 7, 4, 8, p, 1 << 20) == -3          # lda < n
    assert b"argument 3" in lib.tg_last_error()
    assert lib.tg_qr_r(None, p, 8, 0, 8, p, 1 << 20) == -4          # k < 1
    assert lib.tg_qr_r(None, p, 8, 4, 8, None, 1 << 20) == -6       # null ws
    assert lib.tg_qr_r(None, p, 8, 4, 8, p, 16) == -99              # ws too small
    assert b"workspace too small" in lib.tg_last_error()


def test_workspace_size(lib):
    n = 4096
    sizes = [lib.tg_qr_r_workspace_size(k, n) for k in (1, 31, 32, 33, 256, 257, 1000, 2049, 4096)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    # V (32 per row) and one 32 x 32 T per 256-row leaf block: O(k), not O(k n)
    assert sizes[-1] < 8 * (32 * 4096 + 1024 * 16) + 4096
