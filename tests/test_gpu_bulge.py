"""Band -> tridiagonal stage (csrc/bulge.hip, the second half of
torch.linalg.eigh at gptq_utils.py:92) through tg_band_tridiag.

* The dataflow kernel (TG_BULGE_DF=1: per-wave task loops synchronised by
  LDS progress counters) against the step-synchronous kernel (TG_BULGE_DF=0):
  the same tasks with the same arithmetic in the same per-element order, so
  d, e and every reflector record must agree bit for bit -- at widths that
  exercise empty and one-task sweeps (n = 3 .. 65), partial last groups and
  ring wrap-around (n >= 257), and the bench width.
* The tridiagonal's eigenvalues against LAPACK on the band (1e-12 ||B||).
"""
import numpy as np
import pytest
import scipy.linalg as sl
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 32
LDB = 2 * B


def band(n, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for dg in range(min(B, n - 1) + 1):
        v = rng.standard_normal(n - dg)
        A[np.arange(dg, n), np.arange(n - dg)] = v
        A[np.arange(n - dg), np.arange(dg, n)] = v
    return A


def run(lib, A, df, monkeypatch):
    n = A.shape[0]
    monkeypatch.setenv("TG_BULGE_DF", df)
    Ad = torch.from_numpy(A).to(DEV)
    ws = lib.workspace(lib.lib.tg_band_tridiag_workspace_size(n), torch.device(DEV))
    ws.zero_()
    d = torch.empty(n, dtype=torch.float64, device=DEV)
    e = torch.empty(n, dtype=torch.float64, device=DEV)
    lib.call("tg_band_tridiag", lib.stream(), lib.ptr(Ad), n, n, lib.ptr(d), lib.ptr(e),
             lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    # V2 (the reflector records) follows the band storage in the workspace
    nsw, smax = max(1, n - 2), (n - 3) // B + 1 if n >= 3 else 1
    off = -(-n * LDB * 8 // 256) * 256
    v2 = ws[off: off + nsw * smax * B * 8].cpu().numpy().view(np.float64)
    return d.cpu().numpy(), e.cpu().numpy(), v2


@pytest.mark.parametrize("n", [3, 4, 5, 33, 34, 35, 64, 65, 100, 257, 600, 1000, 2049, 4096])
def test_dataflow_bit_identical(n, monkeypatch):
    from gptq_svd_amd import _lib as lib
    A = band(n, n)
    d0, e0, v0 = run(lib, A, "0", monkeypatch)
    d1, e1, v1 = run(lib, A, "1", monkeypatch)
    assert np.isfinite(d1).all()
    assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64))
    assert np.array_equal(e0[:n - 1].view(np.uint64), e1[:n - 1].view(np.uint64))
    assert np.array_equal(v0.view(np.uint64), v1.view(np.uint64))
    if n >= 64:
        w = sl.eigvalsh_tridiagonal(d1, e1[:n - 1])
        ref = sl.eigvalsh(A)
        assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max()


def test_dataflow_repeats(monkeypatch):
    """Run to run: the dataflow schedule changes with timing, the values may not."""
    from gptq_svd_amd import _lib as lib
    A = band(3000, 7)
    ref = run(lib, A, "1", monkeypatch)
    for _ in range(3):
        got = run(lib, A, "1", monkeypatch)
        for a, b in zip(ref, got):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n", [384, 1024])
def test_dataflow_repeats_many(n, monkeypatch):
    """Thousands of launches (round 5: a missing compiler barrier on the LDS
    wait's fast path let ~1 in 1500 launches return a different last 32 (d, e);
    tools/bulge_hunt.py).  At that rate 3000 launches miss it with p ~ 0.14."""
    from gptq_svd_amd import _lib as lib
    monkeypatch.setenv("TG_BULGE_DF", "1")
    Ad = torch.from_numpy(band(n, n)).to(DEV)
    ws = lib.workspace(lib.lib.tg_band_tridiag_workspace_size(n), torch.device(DEV))
    d = torch.empty(n, dtype=torch.float64, device=DEV)
    e = torch.empty(n, dtype=torch.float64, device=DEV)
    ref = None
    bad = 0
    for _ in range(3000 if n <= 384 else 1000):
        lib.call("tg_band_tridiag", lib.stream(), lib.ptr(Ad), n, n, lib.ptr(d), lib.ptr(e),
                 lib.ptr(ws), ws.numel())
        if ref is None:
            ref = (d.clone(), e[:n - 1].clone())
        else:
            bad += int(not (torch.equal(d, ref[0]) and torch.equal(e[:n - 1], ref[1])))
    assert bad == 0


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_tri_guard_quiet(n, monkeypatch, capfd):
    """The tridiagonal guard (csrc/bulge.hip tri_check_kernel: trace and
    squared Frobenius norm of the band preserved by the chase) stays quiet on
    healthy launches, with its residuals far below its 1e-10 bars."""
    import re
    from gptq_svd_amd import _lib as lib
    monkeypatch.setenv("TG_TRI_GUARD_PRINT", "1")
    d, e = run(lib, band(n, n + 3), "1", monkeypatch)[:2]
    assert np.isfinite(d).all() and np.isfinite(e[:n - 1]).all()
    out = capfd.readouterr().err
    m = re.search(r"tri_guard n=(\d+): trace (\S+) frobenius (\S+)", out)
    assert m and int(m.group(1)) == n, out
    print(out.strip())
    assert float(m.group(2)) <= 1e-13 and float(m.group(3)) <= 1e-13


@pytest.mark.parametrize("entry", ["tg_band_tridiag", "tg_eigh_values"])
def test_tri_guard_fires(entry, monkeypatch):
    """A corrupted tridiagonal (TG_TRI_GUARD_CORRUPT=i: d[i] moved by
    1e-3 (1 + |d_i|) on the device after the chase, as a faulty pipeline
    would leave it) fails the invariant check: the call raises and the
    outputs are NaN, so no rank, perm or U is formed from it; the next call
    without the switch is clean again."""
    from gptq_svd_amd import _lib as lib
    n = 700
    A = band(n, 11) if entry == "tg_band_tridiag" else (lambda X: X.T @ X / 1000)(
        np.random.default_rng(5).standard_normal((1000, n)))
    Ad = torch.from_numpy(A).to(DEV)
    if entry == "tg_band_tridiag":
        ws = lib.workspace(lib.lib.tg_band_tridiag_workspace_size(n), torch.device(DEV))
        d = torch.empty(n, dtype=torch.float64, device=DEV)
        e = torch.empty(n, dtype=torch.float64, device=DEV)
        args = lambda: (lib.stream(), lib.ptr(Ad), n, n, lib.ptr(d), lib.ptr(e), lib.ptr(ws),
                        ws.numel())
        outs = lambda: [d, e[:n - 1]]
    else:
        ws = lib.workspace(lib.lib.tg_eigh_workspace_size(n), torch.device(DEV))
        w = torch.empty(n, dtype=torch.float64, device=DEV)
        args = lambda: (lib.stream(), lib.ptr(Ad.clone()), n, n, lib.ptr(w), lib.ptr(ws),
                        ws.numel())
        outs = lambda: [w]
    monkeypatch.setenv("TG_TRI_GUARD_CORRUPT", "37")
    with pytest.raises(RuntimeError, match="invariant check"):
        lib.call(entry, *args())
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs())
    monkeypatch.delenv("TG_TRI_GUARD_CORRUPT")
    lib.call(entry, *args())
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in outs())


@pytest.mark.parametrize("n", [35, 257])
def test_workspace_exact(n):
    """tg_band_tridiag stays inside tg_band_tridiag_workspace_size(n) bytes
    (band storage, reflector records, progress words): with exactly that many
    bytes passed, a poisoned tail behind them is unchanged and the result is
    the one LAPACK gives on the band (1e-12 ||B||, as above)."""
    from gptq_svd_amd import _lib as lib
    A = band(n, n)
    Ad = torch.from_numpy(A).to(DEV)
    size, tail = lib.lib.tg_band_tridiag_workspace_size(n), 4096
    ws = torch.full((size + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    d = torch.empty(n, dtype=torch.float64, device=DEV)
    e = torch.empty(n, dtype=torch.float64, device=DEV)
    lib.call("tg_band_tridiag", lib.stream(), lib.ptr(Ad), n, n, lib.ptr(d), lib.ptr(e),
             lib.ptr(ws), size)
    torch.cuda.synchronize()
    assert bool((ws[size:] == 0xA5).all())
    w = sl.eigvalsh_tridiagonal(d.cpu().numpy(), e[:n - 1].cpu().numpy())
    ref = sl.eigvalsh(A)
    assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max()
