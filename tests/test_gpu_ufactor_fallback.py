"""Householder QR fallback of the U factors (ufactor.hip + hqr.hip, TG_U_QR).

tg_u_factor / tg_u_factor_rx / tg_urx_u11 take U from the Cholesky factor of a
Gram matrix, which squares the condition number; past cond(A[:, :k]) ~ 3e13
the shifted CholeskyQR3 refinement gives up.  The reference's Householder QR
(gptq_utils.py:120) does not, and neither does the library any more: it takes
the factor from tg_qr_r's kernels instead (tg_u_factor_last_path() == 2).

Bars: U within 1e-8 relative Frobenius of LAPACK's sign-normalised R (the
project's U bar) and the residual ||U^T U - A^T A||_F / ||A||_F^2 at most 10x
LAPACK's own on the recovery cases; the bars of test_gpu_conditioning /
test_gpu_solver where their cases are rerun with TG_U_QR=householder.
"""
import logging

import numpy as np
import pytest
import scipy.linalg
import torch

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    import gptq_svd_amd.gptq_utils as g
    return g


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


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


_problems = {}


def problem(*key):
    """factor_problem, computed once per argument tuple and shared (read-only)."""
    if key not in _problems:
        _problems[key] = factor_problem(*key)
    return _problems[key]


def last_path(lib):
    return int(lib.lib.tg_u_factor_last_path())


def u_factor(lib, Vh, S, perm):
    k, n = Vh.shape
    U = torch.empty((k, n), dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_ufactor_workspace_size(n, k), DEV)
    dV, dS, dp = t(Vh), t(S), t(perm)
    lib.call("tg_u_factor", lib.stream(), lib.ptr(dV), n, lib.ptr(dS), lib.ptr(dp), n, k,
             lib.ptr(U), n, lib.ptr(ws), ws.numel())
    return U.cpu().numpy()


def u_factor_rx(lib, Rx):
    k, n = Rx.shape
    U = torch.empty((k, n), dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_ufactor_rx_workspace_size(n, k), DEV)
    dR = t(Rx)
    lib.call("tg_u_factor_rx", lib.stream(), lib.ptr(dR), n, n, k, lib.ptr(U), n, lib.ptr(ws),
             ws.numel())
    return U.cpu().numpy()


def residual(R, A):
    return float(np.linalg.norm(R.T @ R - A.T @ A) / np.linalg.norm(A) ** 2)


@pytest.mark.parametrize("n,k,s", [(200, 160, 7.5), (300, 300, 7.5)])
def test_recovers_where_the_gram_form_breaks_down(lib, monkeypatch, n, k, s):
    Vh, S, perm, _, R = problem(n, k, s, -s, n + k)
    # on the hardware: this input is past the Gram form's reach
    monkeypatch.setenv("TG_U_QR", "gram")
    with pytest.raises(RuntimeError, match="broke down"):
        u_factor(lib, Vh, S, perm)
    monkeypatch.delenv("TG_U_QR")
    U = u_factor(lib, Vh, S, perm)
    assert last_path(lib) == 2
    assert np.all(np.isfinite(U))
    assert np.all(np.tril(U[:, :k], -1) == 0.0)
    assert np.all(np.diag(U) > 0)
    A = (1.0 / S)[:, None] * Vh[:, perm]
    err, res, res_ref = rel(U, R), residual(U, A), residual(R, A)
    print(f"tg_u_factor fallback n={n} k={k} cond=1e{2 * s:g}: |U - R| / |R| = {err:.2e}, "
          f"residual {res:.2e} (LAPACK {res_ref:.2e}, ratio {res / res_ref:.2f})")
    assert err <= 1e-8
    assert res <= 10 * res_ref


@pytest.mark.parametrize("n,k,s_hi,s_lo,tol", [(384, 320, 4.0, -5.0, 1e-5),
                                               (384, 320, 3.0, -3.0, 1e-8),
                                               (512, 256, 1.5, -2.0, 1e-10),
                                               (300, 300, 4.0, -4.0, 1e-8)])
def test_forced_householder_u_factor(lib, monkeypatch, n, k, s_hi, s_lo, tol):
    """The rows and bars of test_gpu_conditioning.test_u_factor_conditioning."""
    monkeypatch.setenv("TG_U_QR", "householder")
    Vh, S, perm, _, R = problem(n, k, s_hi, s_lo, n + k)
    U = u_factor(lib, Vh, S, perm)
    assert last_path(lib) == 2
    assert np.all(np.isfinite(U))
    assert np.allclose(np.tril(U[:, :k], -1), 0.0)
    assert np.all(np.diag(U) > 0)
    err = rel(U, R)
    print(f"tg_u_factor householder n={n} k={k} cond=1e{s_hi - s_lo:g}: {err:.2e}")
    assert err < tol


@pytest.mark.parametrize("n,k,s_hi,s_lo,tol", [(384, 320, 4.0, -5.0, 1e-5),
                                               (384, 320, 3.0, -3.0, 1e-7),
                                               (512, 256, 1.5, -2.0, 1e-8),
                                               (300, 300, 4.0, -4.0, 1e-7)])
def test_forced_householder_u_factor_rx(lib, monkeypatch, n, k, s_hi, s_lo, tol):
    """The rows and bars of test_gpu_conditioning.test_u_factor_rx_conditioning."""
    monkeypatch.setenv("TG_U_QR", "householder")
    _, _, _, Rx, R = problem(n, k, s_hi, s_lo, 7 * n + k)
    U = u_factor_rx(lib, Rx)
    assert last_path(lib) == 2
    assert np.all(np.isfinite(U))
    assert np.all(np.diag(U) > 0)
    err = rel(U, R)
    print(f"tg_u_factor_rx householder n={n} k={k} cond=1e{s_hi - s_lo:g}: {err:.2e}")
    assert err < tol


def test_default_path_unchanged(lib, monkeypatch):
    """A Gram factor that does not break: auto == gram bit for bit, path 0."""
    Vh, S, perm, Rx, _ = problem(512, 256, 1.5, -2.0, 512 + 256)
    U0 = u_factor(lib, Vh, S, perm)
    assert last_path(lib) == 0
    V0 = u_factor_rx(lib, Rx)
    assert last_path(lib) == 0
    monkeypatch.setenv("TG_U_QR", "gram")
    assert np.array_equal(u_factor(lib, Vh, S, perm), U0)
    assert last_path(lib) == 0
    assert np.array_equal(u_factor_rx(lib, Rx), V0)
    assert last_path(lib) == 0


@pytest.mark.parametrize("path", ["kept", "complement"])
@pytest.mark.parametrize("name", ["p_n256_w4a_e4", "p_n512_w4a_e4_b128"] + golden_names("s_"))
def test_goldens_forced_householder(g, monkeypatch, name, path):
    monkeypatch.setenv("TG_U_QR", "householder")
    monkeypatch.setenv("TG_SPECTRAL_PATH", path)
    d = load_golden(name)
    U, R_x, perm, S, k = g.truncated_spectral_factor(t(d["H"]), float(d["eps"]), str(d["method"]))
    assert g.truncated_spectral_factor.last_ufactor == "householder"
    assert k == int(d["k"])
    assert np.array_equal(perm.cpu().numpy(), d["perm"])
    err = rel(U.cpu().numpy(), d["U"])
    taken = g.truncated_spectral_factor.last_path[0]
    print(f"{name} {path}->{taken} householder: |U - U_ref| / |U_ref| = {err:.2e}")
    if name.startswith("p_"):
        tol = 1e-8                      # test_gpu_solver
    else:                               # test_gpu_conditioning
        tol = 1e-4 if path == "complement" and name.startswith("s_n512_w4a_graded") else 1e-5
    assert err < tol


def test_sharded_pieces_forced_householder(lib, monkeypatch):
    from gptq_svd_amd.dist import UrxHip, u_factor_rx_sharded
    monkeypatch.setenv("TG_U_QR", "householder")
    n, k = 1536, 1100
    R = np.linalg.qr(np.random.default_rng(n + k).standard_normal((k, n)), mode="r")
    Rx = t(np.sign(np.diag(R))[:, None] * R)
    sharded = u_factor_rx_sharded(Rx, n, k)
    assert last_path(lib) == 2
    full = UrxHip().full(Rx, n, k)
    assert last_path(lib) == 2
    assert torch.equal(sharded, full)


@pytest.mark.parametrize("mode", [None, "householder"])
def test_nan_still_raises(lib, monkeypatch, mode):
    if mode:
        monkeypatch.setenv("TG_U_QR", mode)
    Vh, S, perm, Rx, _ = problem(128, 96, 1.0, -1.0, 5)
    Vh, Rx = Vh.copy(), Rx.copy()
    Vh[3, 7] = np.nan
    with pytest.raises(RuntimeError, match="broke down"):
        u_factor(lib, Vh, S, perm)
    Rx[2, 50] = np.nan
    with pytest.raises(RuntimeError, match="broke down"):
        u_factor_rx(lib, Rx)


def _inject(g, monkeypatch, message):
    real, state = g.call, {"n": 0}

    def call(name, *args):
        if name == "tg_u_factor_rx":
            state["n"] += 1
            if state["n"] == 1:
                raise RuntimeError(message)
        return real(name, *args)

    monkeypatch.setattr(g, "call", call)


def test_python_rerun_on_complement_breakdown(g, monkeypatch, caplog):
    d = load_golden("p_n512_w4a_e4_b128")
    H, eps, method = t(d["H"]), float(d["eps"]), str(d["method"])
    monkeypatch.setenv("TG_SPECTRAL_PATH", "kept")
    Uk, Rk, pk, _, kk = g.truncated_spectral_factor(H, eps, method)
    monkeypatch.setenv("TG_SPECTRAL_PATH", "complement")
    _inject(g, monkeypatch, "tg_u_factor_rx failed (999): U factor broke down (injected)")
    with caplog.at_level(logging.WARNING):
        U, R_x, perm, _, k = g.truncated_spectral_factor(H, eps, method)
    assert g.truncated_spectral_factor.last_path[0] == "kept"
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1
    assert k == kk
    assert torch.equal(perm, pk) and torch.equal(U, Uk) and torch.equal(R_x, Rk)


def test_python_other_errors_propagate(g, monkeypatch):
    d = load_golden("p_n512_w4a_e4_b128")
    monkeypatch.setenv("TG_SPECTRAL_PATH", "complement")
    _inject(g, monkeypatch, "boom")
    with pytest.raises(RuntimeError, match="boom"):
        g.truncated_spectral_factor(t(d["H"]), float(d["eps"]), str(d["method"]))


def test_python_rerun_then_householder_logs_both(g, monkeypatch, caplog):
    """The rerun's tg_u_factor takes the Householder path: one warning each."""
    d = load_golden("p_n512_w4a_e4_b128")
    monkeypatch.setenv("TG_SPECTRAL_PATH", "complement")
    monkeypatch.setenv("TG_U_QR", "householder")
    _inject(g, monkeypatch, "tg_u_factor_rx failed (999): U factor broke down (injected)")
    with caplog.at_level(logging.WARNING):
        U, _, perm, _, k = g.truncated_spectral_factor(t(d["H"]), float(d["eps"]), str(d["method"]))
    assert g.truncated_spectral_factor.last_path[0] == "kept"
    assert g.truncated_spectral_factor.last_ufactor == "householder"
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 2
    assert k == int(d["k"]) and np.array_equal(perm.cpu().numpy(), d["perm"])
    assert rel(U.cpu().numpy(), d["U"]) < 1e-8
