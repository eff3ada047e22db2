"""Streamed fill of the pivot order (csrc/pivot.hip: TG_PIV_STREAM, default on).

With the switch on, fill workers in the piv_sel_kernel launch compute the
panel's L columns and Schur diagonals step by step behind the selector, and
piv_fill_kernel only fills what they left.  Nothing may change: every case
compares tg_pivoted_factor_complement with TG_PIV_STREAM=0 against
TG_PIV_STREAM=1 on the same Hessian: perm and R_x with torch.equal, the
TG_PIV_STATS counts for equality.  One shape does the same for
tg_pivoted_factor, and one compares U of tg_u_factor_rx as well.

Cases, the smallest at which each mechanism can go wrong:
  n96        n = 96, k = 70: one worker chunk (the second has 32 rows), k not a
             multiple of 32, last panel short;
  n257       n = k = 257: n not a multiple of 64, a chunk with one valid row;
  n1024      n = 1024, k = 700: several panels, several worker chunks;
  lev256     the same at TG_PIV_LEVEL=256: many panels ended early by the tau
             rule (asserted from the stats), so tn < 32 is really taken;
  lev1024    the same at TG_PIV_LEVEL=1024: no panel is streamed, the workers
             leave at once and the net launch fills everything;
  budget0    the same with TG_PIV_STREAM_BUDGET=0: every worker gives up at
             once, the publisher still writes the records, the net fills all;
  dup512     n = 512 with dead and duplicated channels (tests/degenerate_ref):
             equal diagonals, ties broken by position, candidates at -inf.

The preselected candidates (TG_PIV_PRESEL) of the same proposal are not part
of the library, so there is no second switch to combine and no n = 9000 case.
"""
import functools
import re

import numpy as np
import pytest
import torch

import degenerate_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {
    "n96": (96, 70, {}),
    "n257": (257, 257, {}),
    "n1024": (1024, 700, {}),
    "lev256": (1024, 700, {"TG_PIV_LEVEL": "256"}),
    "lev1024": (1024, 700, {"TG_PIV_LEVEL": "1024"}),
    "budget0": (1024, 700, {"TG_PIV_STREAM_BUDGET": "0"}),
    "dup512": (512, None, {}),
}


@functools.lru_cache(maxsize=None)
def _hessian(n):
    """Random Gram matrix with a decaying spectrum (read-only, shared)."""
    if n == 512:
        X, dead, pairs = dr.degenerate_x(768, n, 9, 14, 512)
        H = dr.hessian(X, pairs)
        k = dr.structural_rank(n, dead, pairs)
    else:
        rng = np.random.default_rng(n)
        # singular values 1 .. 1e-2 in a random basis: the spectrum decays, the
        # diagonals stay close to each other (so the tau rule is live)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        X = (rng.standard_normal((3 * n // 2, n)) * np.logspace(0.0, -2.0, n)) @ Q.T
        H = X.T @ X / X.shape[0]
        H = 0.5 * (H + H.T)
        k = None
    H.setflags(write=False)
    return H, k


def _stats(err):
    m = re.search(r"pivot stats: .*", err)
    assert m, f"no TG_PIV_STATS line in {err!r}"
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", m.group(0))}


def _complement(H, k):
    from gptq_svd_amd import _lib as lib
    n = H.shape[0]
    Hd = torch.from_numpy(np.array(H)).to(DEV)
    perm = torch.empty(n, dtype=torch.int64, device=DEV)
    Rx = torch.empty((k, n), dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_pivot_workspace_size(n, k), torch.device(DEV))
    lib.call("tg_pivoted_factor_complement", lib.stream(), lib.ptr(Hd), n, None, n, None, 0, n, k,
             lib.ptr(perm), lib.ptr(Rx), n, lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return perm, Rx


def _both(monkeypatch, capfd, env, solve):
    """solve() with TG_PIV_STREAM=0 and =1 -> [(outputs, stats)] * 2."""
    monkeypatch.setenv("TG_PIV_STATS", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    out = []
    for stream in ("0", "1"):
        monkeypatch.setenv("TG_PIV_STREAM", stream)
        capfd.readouterr()
        res = solve()
        out.append((res, _stats(capfd.readouterr().err)))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_stream_bit_identical(case, monkeypatch, capfd):
    n, k, env = CASES[case]
    H, kd = _hessian(n)
    k = kd if k is None else k
    (base, st0), (got, st1) = _both(monkeypatch, capfd, env, lambda: _complement(H, k))
    with capfd.disabled():
        print(f"\n{case}: {st1}", end="")
    assert st0 == st1, (st0, st1)
    assert st0["panels"] >= -(-k // 32)
    if case == "lev256":
        assert st1["early"] > 0 and st1["level256"] == st1["panels"], st1
    if case == "lev1024":
        assert st1["level1024"] == st1["panels"], st1
    assert torch.equal(got[0], base[0]), "perm differs"
    assert torch.equal(got[1], base[1]), "R_x differs"
    assert sorted(got[0].tolist()) == list(range(n))
    assert torch.isfinite(got[1]).all()
    if case == "n1024":  # U from the two R_x
        from gptq_svd_amd import _lib as lib
        us = []
        for Rx in (base[1], got[1]):
            U = torch.empty((k, n), dtype=torch.float64, device=DEV)
            ws = lib.workspace(lib.lib.tg_ufactor_rx_workspace_size(n, k), torch.device(DEV))
            lib.call("tg_u_factor_rx", lib.stream(), lib.ptr(Rx), n, n, k, lib.ptr(U), n,
                     lib.ptr(ws), ws.numel())
            us.append(U)
        torch.cuda.synchronize()
        assert torch.equal(us[0], us[1]), "U differs"


def test_stream_kept_path(monkeypatch, capfd):
    """tg_pivoted_factor (H_k = (S Vh)^T (S Vh)) on n = 300, k = 200."""
    from gptq_svd_amd import _lib as lib
    n, k = 300, 200
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Vh = torch.from_numpy(np.ascontiguousarray(Q.T[:k])).to(DEV)
    S = torch.from_numpy(np.logspace(0.0, -2.0, k)).to(DEV)

    def solve():
        perm = torch.empty(n, dtype=torch.int64, device=DEV)
        Rx = torch.empty((k, n), dtype=torch.float64, device=DEV)
        ws = lib.workspace(lib.lib.tg_pivot_workspace_size(n, k), torch.device(DEV))
        lib.call("tg_pivoted_factor", lib.stream(), lib.ptr(Vh), n, lib.ptr(S), n, k, lib.ptr(perm),
                 lib.ptr(Rx), n, lib.ptr(ws), ws.numel())
        torch.cuda.synchronize()
        return perm, Rx

    (base, st0), (got, st1) = _both(monkeypatch, capfd, {}, solve)
    assert st0 == st1, (st0, st1)
    assert torch.equal(got[0], base[0]), "perm differs"
    assert torch.equal(got[1], base[1]), "R_x differs"
