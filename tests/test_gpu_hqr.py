"""tg_qr_r: blocked Householder QR (R only, TSQR tree, hqr.hip) against LAPACK.

Bars: R within 1e-8 relative Frobenius of np.linalg.qr(mode="r"),
sign-normalised (the project's U bar); the residual
||R^T R - A^T A||_F / ||A||_F^2 at most 10x the same quantity for LAPACK's R
(the margin covers a different summation order); strict lower triangle
exactly 0; diagonal > 0; columns n .. lda-1 untouched.
"""
import numpy as np
import pytest
import scipy.linalg
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


def factor_problem(n, k, s_hi, s_lo, seed):
    """Orthonormal Vh (k x n), S log-spaced s_hi .. s_lo (cond(A) = 10^(s_hi - s_lo)),
    perm and R_x from LAPACK dgeqp3 of diag(S) Vh, and the reference U =
    sign-normalised R of Householder QR(diag(1/S) Vh[:, perm])."""
    rng = np.random.default_rng(seed)
    Vh = np.linalg.qr(rng.standard_normal((n, n)))[0][:, :k].T.copy()
    S = np.logspace(s_hi, s_lo, k)
    _, Rx, perm = scipy.linalg.qr(S[:, None] * Vh, pivoting=True, mode="economic")
    Rx = Rx * np.sign(np.diag(Rx))[:, None]
    R = np.linalg.qr((1.0 / S)[:, None] * Vh[:, perm], mode="r")
    R = R * np.sign(np.diag(R))[:, None]
    return Vh, S, perm.astype(np.int64), Rx, R


def qr_r(lib, A, lda=None):
    """tg_qr_r on a copy of A padded to lda columns of sentinels; returns the
    whole k x lda buffer."""
    k, n = A.shape
    lda = n if lda is None else lda
    buf = np.full((k, lda), SENTINEL)
    buf[:, :n] = A
    d = torch.from_numpy(buf).to(DEV)
    ws = lib.workspace(lib.lib.tg_qr_r_workspace_size(k, n), DEV)
    lib.call("tg_qr_r", lib.stream(), lib.ptr(d), lda, k, n, lib.ptr(ws), ws.numel())
    return d.cpu().numpy()


def lapack_r(A):
    R = np.linalg.qr(A, mode="r")
    s = np.where(np.diag(R) < 0, -1.0, 1.0)
    return R * s[:, None]


def residual(R, A):
    return float(np.linalg.norm(R.T @ R - A.T @ A) / np.linalg.norm(A) ** 2)


def check(tag, out, A, full_rank=True):
    k, n = A.shape
    R = out[:, :n]
    assert np.all(np.isfinite(R))
    assert np.all(out[:, n:] == SENTINEL)
    assert np.all(np.tril(R[:, :k], -1) == 0.0)
    ref = lapack_r(A)
    res, res_ref = residual(R, A), residual(ref, A)
    print(f"{tag}: residual {res:.2e} (LAPACK {res_ref:.2e}, ratio "
          f"{res / res_ref if res_ref else float('nan'):.2f})", end="")
    if full_rank:
        err = float(np.linalg.norm(R - ref) / np.linalg.norm(ref))
        print(f", |R - R_lapack| / |R_lapack| = {err:.2e}")
        assert np.all(np.diag(R) > 0)
        assert err <= 1e-8
    else:
        print()
        assert np.all(np.diag(R) >= 0)
    assert res <= 10 * res_ref


@pytest.mark.parametrize("k,n,lda", [(1, 37, 37), (20, 50, 50), (33, 33, 34), (64, 1500, 1500),
                                     (257, 300, 301), (545, 608, 608), (2100, 2177, 2178)])
def test_gaussian(lib, k, n, lda):
    A = np.random.default_rng(k + n).standard_normal((k, n))
    check(f"gaussian {k}x{n} lda={lda}", qr_r(lib, A, lda), A)


@pytest.mark.parametrize("n,k", [(200, 160), (300, 300), (608, 545)])
def test_graded(lib, n, k):
    Vh, S, perm, _, _ = factor_problem(n, k, 7.5, -7.5, n + k)
    A = (1.0 / S)[:, None] * Vh[:, perm]
    check(f"graded n={n} k={k} cond=1e15", qr_r(lib, A), A)


def test_rank_deficient(lib):
    A = np.random.default_rng(96 + 128).standard_normal((96, 128))
    A[:, 5] = 0.0
    A[:, 40] = A[:, 3]
    check("rank-deficient 96x128", qr_r(lib, A), A, full_rank=False)


def test_nan_raises_then_clean_call_passes(lib):
    A = np.random.default_rng(300 + 400).standard_normal((300, 400))
    B = A.copy()
    B[170, 45] = np.nan
    with pytest.raises(RuntimeError, match="broke down"):
        qr_r(lib, B)
    check("after NaN 300x400", qr_r(lib, A), A)


def test_deterministic(lib):
    A = np.random.default_rng(545 + 700).standard_normal((545, 700))
    assert np.array_equal(qr_r(lib, A, 701), qr_r(lib, A, 701))


def test_nan_in_trailing_column_raises(lib):
    """A NaN / Inf in a column >= k never meets a column norm; the finished R
    is checked for it."""
    A = np.random.default_rng(64 + 200).standard_normal((64, 200))
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[40, 150] = bad
        with pytest.raises(RuntimeError, match="broke down"):
            qr_r(lib, B)


@pytest.mark.parametrize("e", [565, -565])
def test_extreme_scale(lib, e):
    """Entries near 1e170 / 1e-170: their squares overflow / underflow, the
    scaled column norm does not (power-of-two scale: R scales exactly)."""
    A = np.random.default_rng(300 + 333).standard_normal((300, 333))
    out = qr_r(lib, A * 2.0 ** e)
    check(f"gaussian 300x333 scaled 2^{e}", out * 2.0 ** -e, A)
