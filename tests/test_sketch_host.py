"""CPU: the sketch entry points' ABI, argument checks and public names, plus a
numpy restatement of omega(seed, r, g) (include/truncgptq.h: Philox4x32-10 and
Box-Muller, here in float64) that tests/test_gpu_sketch.py compares the device
values against.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "truncgptq.h")
LIB = os.path.join(ROOT, "gptq-svd_amd", "libtruncgptq.so")

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words; key: two ints.  Returns the
    four output words (uint64 arrays holding 32-bit values)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def omega_ref(seed, rows, tokens):
    """omega(seed, r, g) for r in `rows`, g in `tokens` (global token indices,
    Python ints or an integer array), float64, shape (len(rows), len(tokens))."""
    r = np.asarray(rows, dtype=np.uint64)[:, None]
    g = np.asarray([int(t) for t in tokens], dtype=np.uint64)[None, :]
    r, g = np.broadcast_arrays(r, g)
    rg = (r >> np.uint64(7)) * np.uint64(32) + (r & np.uint64(31))
    j = ((r >> np.uint64(5)) & np.uint64(3)).astype(np.int64)
    x = philox4x32_10([g & MASK, g >> np.uint64(32), rg, np.zeros_like(g)],
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    xa = np.where(j < 2, x[0], x[2])
    xb = np.where(j < 2, x[1], x[3])
    u1 = ((xa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24   # (0, 1]
    u2 = (xb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                    # [0, 1)
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.where(j % 2 == 0, rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2))


def test_philox_known_answers():
    """The published Philox4x32-10 known-answer vectors (Random123 kat_vectors)."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        got = philox4x32_10([np.array([w], dtype=np.uint64) for w in ctr], key)
        assert tuple(int(w[0]) for w in got) == want


def test_omega_ref_is_a_pure_function_of_row_and_token():
    a = omega_ref(5, range(300), range(10, 20))
    assert np.array_equal(a[:70], omega_ref(5, range(70), range(10, 20)))
    assert np.array_equal(a[:, 3:], omega_ref(5, range(300), range(13, 20)))
    assert not np.array_equal(a, omega_ref(6, range(300), range(10, 20)))
    assert np.isfinite(a).all() and len(np.unique(a)) == a.size
    big = omega_ref(5, range(4), [2 ** 32 - 1, 2 ** 32])   # the counter's second word
    assert np.isfinite(big).all() and not np.array_equal(big[:, 0], big[:, 1])


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "gptq-svd_amd"), "-j8"], check=True)
    L = ctypes.CDLL(LIB)
    vp, i, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    L.tg_sketch_accum.argtypes = [vp, vp, i, i64, i, i64, u64, i64, vp, i, i64]
    L.tg_sketch_accum.restype = i
    L.tg_sketch_omega.argtypes = [vp, u64, i64, i, i64, vp, i64]
    L.tg_sketch_omega.restype = i
    L.tg_last_error.restype = ctypes.c_char_p
    return L


def test_header_declares_and_library_exports(lib):
    assert {"tg_sketch_omega", "tg_sketch_accum"} <= declared()
    assert hasattr(lib, "tg_sketch_omega") and hasattr(lib, "tg_sketch_accum")
    import gptq_svd_amd._lib as L
    assert {"tg_sketch_omega", "tg_sketch_accum"} <= set(L.EXPORTED)


def test_argument_errors_without_device(lib):
    """-(1-based argument index), before any device work (there is no device
    here): X=2, x_dtype=3, T=4, n=5, ldx=6, seed=7, t0=8, Y=9, rank=10, ldy=11."""
    p = ctypes.c_void_p(64)

    def accum(X=p, dt=0, T=8, n=16, ldx=16, t0=0, Y=p, rank=4, ldy=16):
        return lib.tg_sketch_accum(None, X, dt, T, n, ldx, 1, t0, Y, rank, ldy)

    assert accum(rank=0) == -10 and b"argument 10" in lib.tg_last_error()
    assert accum(rank=-3) == -10
    assert accum(n=0) == -5
    assert accum(ldx=15) == -6
    assert accum(ldy=15) == -11
    assert accum(dt=3) == -3 and accum(dt=-1) == -3 and accum(dt=7) == -3
    assert accum(X=None) == -2 and b"argument 2" in lib.tg_last_error()
    assert accum(T=-1) == -4
    assert accum(t0=-1) == -8
    assert accum(Y=None) == -9
    # T = 0: nothing to do, and X may be null
    assert accum(T=0) == 0
    assert accum(T=0, X=None) == 0
    assert accum(T=0, rank=0) == -10

    def omega(t0=0, rank=4, T=8, Om=p, ldo=8):
        return lib.tg_sketch_omega(None, 1, t0, rank, T, Om, ldo)

    assert omega(t0=-1) == -3
    assert omega(rank=0) == -4
    assert omega(T=-1) == -5
    assert omega(Om=None) == -6
    assert omega(ldo=7) == -7
    assert omega(T=0, Om=None) == 0


def test_package_exports():
    import gptq_svd_amd
    import gptq_svd_amd.gptq_utils as g
    for name in ("Sketcher", "process_sketch"):
        assert name in g.__all__
        assert getattr(gptq_svd_amd, name) is getattr(g, name)
    import gptq_svd_amd.harness as h
    assert h.Sketcher is g.Sketcher and h.process_sketch is g.process_sketch


def test_no_cpu_fallback():
    import torch
    import gptq_svd_amd.gptq_utils as g
    with pytest.raises(RuntimeError):
        g.Sketcher(torch.nn.Linear(8, 4), 16, device="cpu")
    with pytest.raises(RuntimeError):
        g.process_sketch(torch.zeros(16, 8))
    with pytest.raises(ValueError):
        g.process_sketch(torch.zeros(16, 8), threshold_method="bogus")


def test_mode_checks(monkeypatch):
    import torch
    import gptq_svd_amd.harness as h
    model = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="mode must be"):
        h.quantize_model(model, [], mode="bogus")
    # a process group of two ranks: sketch mode refuses before it touches the model
    monkeypatch.setattr(h, "_world", lambda pg=None: (2, 0))
    with pytest.raises(ValueError, match="mode 'svd' is single-process"):
        h.quantize_model(model, [], mode="svd", pg=object())
