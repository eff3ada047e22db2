"""Streamed fill of the pivot order (csrc/pivot.hip piv_stream_worker): a numpy
replay of the bookkeeping a worker does per published step against the
end-of-panel mapping piv_fill_kernel uses.  CPU only.

piv_fill_kernel runs after the panel: the thread at final position x >= ps
takes row perm[x], its compact index oidx[x - ps] = (panel-start position) - ps
in the panel's H_k, and writes its LT column x - ps2 when x >= ps2 = ps + tn.
A worker thread is keyed the other way round: it owns the row at panel-start
position x0, so its compact index is x0 - ps, and it has to arrive at the
row's final position by following the published swaps (step t swaps positions
i = ps + t and q).  Both must name the same (row, compact index, final
position, LT column) for every row unpivoted at the panel start, and the rows
pivoted in the panel must end at ps + t with no LT column.

The net launch fills exactly the rows whose panel-start chunk (compact index
// 64) no worker marked; with any subset of chunks marked, workers and net
together must cover every row once.

Cases: random pivot sequences with full panels, panels ended early (tn < 32),
q = i (no swap), pivots that were swapped away from position i earlier in the
panel, a panel reaching the last row, and n - ps not a multiple of 64.
"""
import numpy as np
import pytest

PB = 32
CHUNK = 64


def panel(rng, n, ps, tn, p_noswap):
    """A panel's swaps on a random panel-start perm -> (perm0, perm1, prow, pq)."""
    perm0 = rng.permutation(n)
    perm = perm0.copy()
    prow, pq = [], []
    for t in range(tn):
        i = ps + t
        q = i if rng.random() < p_noswap else int(rng.integers(i, n))
        perm[i], perm[q] = perm[q], perm[i]
        prow.append(int(perm[i]))
        pq.append(q)
    return perm0, perm, prow, pq


def fill_mapping(n, ps, tn, perm0, perm1):
    """piv_fill_kernel: row -> (compact index, final position, LT column or -1)."""
    pos0 = np.empty(n, dtype=np.int64)
    pos0[perm0] = np.arange(n)
    ps2 = ps + tn
    out = {}
    for x in range(ps, n):
        r = int(perm1[x])
        out[r] = (int(pos0[r]) - ps, x, x - ps2 if x >= ps2 else -1)
    return out


def worker_mapping(n, ps, tn, perm0, prow, pq):
    """piv_stream_worker: the same triple from per-step tracking."""
    ps2 = ps + tn
    out = {}
    for x0 in range(ps, n):
        r = int(perm0[x0])
        pos, done = x0, False
        for t in range(tn):
            i, q = ps + t, pq[t]
            act, isp = not done, prow[t] == r
            if act and isp:
                pos = i
            elif pos == i and q != i:
                pos = q
            done = done or (act and isp)
        assert done == (pos < ps2), (r, pos, done)
        out[r] = (x0 - ps, pos, pos - ps2 if pos >= ps2 else -1)
    return out


@pytest.mark.parametrize("n,ps,tn,p_noswap,seed", [
    (96, 0, 32, 0.2, 0),       # first panel, one full and one short chunk
    (96, 64, 6, 0.2, 1),       # last short panel, k % 32 != 0
    (257, 225, 32, 0.0, 2),    # the panel reaches the last row (k = n)
    (257, 192, 32, 0.5, 3),    # a chunk with one valid row (n - ps = 65)
    (1024, 320, 17, 0.1, 4),   # ended early by the tau rule
    (1024, 320, 1, 1.0, 5),    # one step, q = i
    (300, 10, 32, 1.0, 6),     # no swap at all
    (300, 10, 32, 0.0, 7),     # every step swaps
])
def test_worker_tracking_matches_fill(n, ps, tn, p_noswap, seed):
    rng = np.random.default_rng(seed)
    for _ in range(20):
        perm0, perm1, prow, pq = panel(rng, n, ps, tn, p_noswap)
        ref = fill_mapping(n, ps, tn, perm0, perm1)
        got = worker_mapping(n, ps, tn, perm0, prow, pq)
        assert got == ref
        # pivots sit at ps + t, and the LT columns are a permutation of 0 .. n - ps2 - 1
        for t in range(tn):
            assert got[prow[t]][1] == ps + t
        cols = sorted(c for _, _, c in got.values() if c >= 0)
        assert cols == list(range(n - ps - tn))


@pytest.mark.parametrize("n,ps,tn,seed", [(96, 0, 32, 0), (257, 192, 32, 1), (1024, 320, 17, 2)])
def test_net_covers_unmarked_rows_once(n, ps, tn, seed):
    rng = np.random.default_rng(100 + seed)
    perm0, perm1, _, _ = panel(rng, n, ps, tn, 0.2)
    ref = fill_mapping(n, ps, tn, perm0, perm1)
    nchunk = -(-(n - ps) // CHUNK)
    for _ in range(10):
        marked = rng.random(nchunk) < 0.5
        by_worker = {int(perm0[x0]) for x0 in range(ps, n) if marked[(x0 - ps) // CHUNK]}
        by_net = {r for r, (oi, _, _) in ref.items() if not marked[oi // CHUNK]}
        assert not by_worker & by_net
        assert by_worker | by_net == set(ref)
