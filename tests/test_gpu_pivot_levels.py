"""Candidate levels of the pivot order (piv_sel_kernel: 256, 512 or 1024
candidates per panel, chosen on the device or forced with TG_PIV_LEVEL).

tg_pivoted_factor_complement with nc = 0 (greedy diagonal pivoting on
H_k = H) against tests/test_complement_math.pivoted_cholesky, every case with
TG_PIV_LEVEL unset (adaptive), 256, 512 and 1024.  The tau rule makes the
pivot choice independent of the candidate count, so the bars are the same at
every setting: perm identical to the CPU reference (hence across settings),
R_x relative Frobenius <= 1e-10.

Cases, the smallest at which each path can go wrong:
  below     n = 200, k = 150: fewer rows than any level, tau = -inf;
  above256  n = 300, k = 260 and
  above512  n = 600, k = 500: just above a level, its tau live from panel one;
  full      n = 1100 = k: above 1024, full rank, k % 32 != 0, n % 64 != 0;
  ties      n = 640, every column duplicated, k = 250: exact ties by position;
  groups    60 groups of 8 near-identical heavy columns + 400 small, k = 200:
            panels end early, so the adaptive run escalates and the forced-256
            run needs more panels than the forced-1024 run (TG_PIV_STATS);
  deficient X with 180 rows, n = 400, k = 180: candidates exhausted at -inf.

Each case builder checks on the CPU that, outside the intended exact ties,
the chosen Schur diagonal leads the runner-up by a relative gap >= 1e-9 at
every step, so a last-bit difference in R_x cannot legitimately reorder
pivots.
"""
import functools
import re

import numpy as np
import pytest
import torch

from test_complement_math import pivoted_cholesky

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = [None, "256", "512", "1024"]
MIN_GAP = 1e-9


def _min_gap(H, k, order, Rx_ref, exact_ties):
    """Smallest relative gap (chosen - runner-up) / chosen over the reference's
    k steps, from its own factor: the Schur diagonal before step i is
    diag(H) - sum_{l < i} L[:, l]^2 and the rows still unpivoted are
    order[i:].  With exact_ties, diagonals equal to the chosen one (the
    duplicate column) do not count as runner-up."""
    L = np.empty((H.shape[0], k))
    L[order] = Rx_ref.T
    d = np.diagonal(H).copy()
    gap = np.inf
    for i in range(k):
        top, rest = d[order[i]], d[order[i + 1:]]
        if exact_ties:
            rest = rest[rest != top]
        if rest.size:
            gap = min(gap, (top - rest.max()) / top)
        d -= L[:, i] ** 2
    return gap


@functools.lru_cache(maxsize=None)
def _case(kind):
    rng = np.random.default_rng(11)
    ties = False
    if kind == "below":
        n, k = 200, 150
        X = rng.standard_normal((300, n))
    elif kind == "above256":
        n, k = 300, 260
        X = rng.standard_normal((400, n))
    elif kind == "above512":
        n, k = 600, 500
        X = rng.standard_normal((800, n))
    elif kind == "full":
        n, k = 1100, 1100
        X = rng.standard_normal((1500, n))
    elif kind == "ties":
        n, k, ties = 640, 250, True
        X = np.repeat(rng.standard_normal((500, n // 2)), 2, axis=1)
    elif kind == "groups":
        ng, g, nsmall = 60, 8, 400
        # 300 rows: with so few, a step takes enough off the small columns'
        # diagonals that 256 candidates lose more steps than the last panel's
        # slack (k = 6 * 32 + 8), so the forced-256 run needs an eighth panel
        base = 10.0 * rng.standard_normal((300, ng))
        heavy = np.repeat(base, g, axis=1) + 1e-3 * rng.standard_normal((300, ng * g))
        X = np.concatenate([heavy, rng.standard_normal((300, nsmall))], axis=1)
        X = X[:, rng.permutation(X.shape[1])]
        n, k = X.shape[1], 200
    else:  # deficient
        n, k = 400, 180
        X = rng.standard_normal((180, n))
    H = X.T @ X / X.shape[0]
    order, Rx_ref = pivoted_cholesky(H, k)
    gap = _min_gap(H, k, order, Rx_ref, ties)
    assert gap >= MIN_GAP, f"{kind}: reference gap {gap:.3e} < {MIN_GAP}: choose another seed"
    H.setflags(write=False)
    order.setflags(write=False)
    Rx_ref.setflags(write=False)
    return H, k, order, Rx_ref


def _solve(H, k):
    from gptq_svd_amd import _lib as lib
    n = H.shape[0]
    Hd = torch.from_numpy(np.array(H)).to(DEV)
    perm = torch.empty(n, dtype=torch.int64, device=DEV)
    Rx = torch.empty((k, n), dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_pivot_workspace_size(n, k), torch.device(DEV))
    lib.call("tg_pivoted_factor_complement", lib.stream(), lib.ptr(Hd), n, None, n, None, 0, n, k,
             lib.ptr(perm), lib.ptr(Rx), n, lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return perm.cpu().numpy(), Rx.cpu().numpy()


def _stats(err):
    m = re.search(r"pivot stats: .*", err)
    assert m, f"no TG_PIV_STATS line in {err!r}"
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", m.group(0))}


@pytest.mark.parametrize("kind", ["below", "above256", "above512", "full", "ties", "groups",
                                  "deficient"])
def test_pivot_levels(kind, monkeypatch, capfd):
    H, k, order, Rx_ref = _case(kind)
    monkeypatch.setenv("TG_PIV_STATS", "1")
    stats, perms = {}, {}
    for level in LEVELS:
        if level is None:
            monkeypatch.delenv("TG_PIV_LEVEL", raising=False)
        else:
            monkeypatch.setenv("TG_PIV_LEVEL", level)
        capfd.readouterr()
        p, Rx = _solve(H, k)
        stats[level] = _stats(capfd.readouterr().err)
        with capfd.disabled():
            print(f"\n{kind} level={level}: {stats[level]}", end="")
        assert np.array_equal(p[:k], order[:k]), \
            f"level {level}: first mismatch at {np.argmax(p[:k] != order[:k])}"
        assert np.array_equal(p, order), f"level {level}: dgeqp3 tail order differs"
        err = np.linalg.norm(Rx - Rx_ref) / np.linalg.norm(Rx_ref)
        with capfd.disabled():
            print(f" R_x error {err:.3e}", end="")
        assert err <= 1e-10, (level, err)
        perms[level] = p
    for level in LEVELS[1:]:
        assert np.array_equal(perms[level], perms[None]), f"perm at level {level} != adaptive"
    for level, name in (("256", "level256"), ("512", "level512"), ("1024", "level1024")):
        assert stats[level][name] == stats[level]["panels"], (level, stats[level])
    if kind == "groups":
        assert stats[None]["escalations"] >= 1, stats[None]
        assert stats["256"]["panels"] > stats["1024"]["panels"], (stats["256"], stats["1024"])
