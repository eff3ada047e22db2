"""Inputs and host references for Hessians with dead and duplicated channels
(plain numpy; used by test_degenerate_ref.py on the CPU and by
test_gpu_degenerate.py).

A dead input channel (identically zero, e.g. a post-ReLU feature that never
fires) makes row and column j of H = X^T X / N exactly zero.  A duplicated
channel (padded or tied features) makes two rows of H identical.  Both give H
an exact null space of dimension dead + pairs in the middle of an otherwise
dense, well conditioned matrix.

The pivot choice between the two members of a pair is arbitrary, so U and R_x
are compared with `factors_given_perm`: the reference's factors for a perm that
is given instead of recomputed.
"""
import functools

import numpy as np

from oracle import oracle as o

F32 = np.float32


def degenerate_x(N, n, n_dead, n_pairs, seed):
    """fp16 X (N x n) with n_dead zero columns and n_pairs duplicated columns
    at scattered positions.  -> (X, dead sorted int64, pairs [(a, b)]) with
    X[:, b] == X[:, a]."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, n), dtype=F32)
    p = rng.permutation(n)
    dead = np.sort(p[:n_dead]).astype(np.int64)
    rest = p[n_dead:n_dead + 2 * n_pairs]
    pairs = [(int(rest[2 * i]), int(rest[2 * i + 1])) for i in range(n_pairs)]
    for a, b in pairs:
        X[:, b] = X[:, a]
    X[:, dead] = 0.0
    return X.astype(np.float16), dead, pairs


def hessian(X, pairs=()):
    """float64 X^T X / N.  Row and column b of every pair (a, b) are copied
    from a, so the ties in H are exact whatever the host BLAS does."""
    Xd = np.asarray(X, dtype=np.float64)
    H = Xd.T @ Xd / Xd.shape[0]
    H = 0.5 * (H + H.T)
    for a, b in pairs:
        H[b, :] = H[a, :]
        H[:, b] = H[:, a]
    return H


def structural_rank(n, dead, pairs):
    return n - len(dead) - len(pairs)


def factors_given_perm(H, k, perm):
    """(U, R_x) of oracle.process_hessian_alt (oracle.py:104-118) for a given
    perm: eigh, S = sqrt(max(L, 1e-12)) descending, then the sign-normalised R
    factors of QR(diag(1/S_k) Vh_k[:, perm]) and QR(diag(S_k) Vh_k[:, perm]).
    Unique when the leading k x k block is nonsingular, and independent of the
    basis chosen inside an eigenvalue cluster."""
    Hd = np.asarray(H, dtype=np.float64)
    perm = np.asarray(perm, dtype=np.int64)
    L, V = np.linalg.eigh(Hd)
    S = np.sqrt(np.maximum(L, 1e-12))[::-1].copy()
    Vh = V.T[::-1].copy()
    S_k = S[:k]
    Vp = Vh[:k][:, perm]
    _, Ru = np.linalg.qr((1.0 / S_k)[:, None] * Vp, mode="reduced")
    _, Rx = np.linalg.qr(S_k[:, None] * Vp, mode="reduced")
    U = Ru * np.sign(np.diagonal(Ru))[:, None]
    R_x = Rx * np.sign(np.diagonal(Rx))[:, None]
    return U, R_x


def rtn(W, bits, group, sym):
    """Round to nearest on the static grid, dequantised to float32: the tail
    rule of the solver (gptq_utils.py:552-553) applied to every column."""
    W = np.asarray(W, dtype=F32)
    n = W.shape[1]
    min_q, max_q = o.qrange(bits, sym)
    scale, zero = o.find_params(W, bits, group, sym)
    s, z = o.expand_params(scale, zero, n, group)
    q = np.clip(np.rint(W / s + z), F32(min_q), F32(max_q))
    return ((q - z) * s).astype(F32)


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check_perm(perm, k, n, dead, pairs):
    """perm is a permutation of range(n) whose first k entries hold no dead
    index and exactly one index of every pair."""
    perm = np.asarray(perm)
    assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation"
    head = set(perm[:k].tolist())
    assert not head & set(np.asarray(dead).tolist()), "a dead channel was pivoted"
    for a, b in pairs:
        assert (a in head) != (b in head), f"pair ({a}, {b}): not exactly one member kept"


# ---------------------------------------------------------------------------
# eigensolver cases
# ---------------------------------------------------------------------------
# name -> (n, dead, pairs, seed).  The band reduction's Householder panels mix
# the top 32 rows of every panel, so a zero or repeated column survives only
# until the panel before its own: the one panel that is factored with an
# exactly singular Gram matrix is the first (columns 0 .. 31).  The seeds are
# the first from 100 on that put a dead column, a whole pair, or both there
# (test_degenerate_ref.py checks it).
EIGH_X = {"dead200": (200, 7, 0, 103), "dup200": (200, 0, 5, 120), "both200": (200, 7, 5, 104),
          "both600": (600, 20, 12, 131)}


def eigh_x(name):
    n, nd, npair, seed = EIGH_X[name]
    return degenerate_x(3 * n // 2, n, nd, npair, seed)


def _eigh_case(name):
    if name in EIGH_X:
        X, _, pairs = eigh_x(name)
        return hessian(X, pairs)
    rng = np.random.default_rng(len(name) + 40)
    if name == "diag0":
        d = np.repeat(np.linspace(0.0, 2.0, 20), 5)
        rng.shuffle(d)
        d[rng.permutation(100)[:10]] = 0.0
        return np.diag(d)
    if name == "rank1":
        x = rng.standard_normal(150)
        return np.outer(x, x)
    if name == "cI":
        return 2.5 * np.eye(70)
    if name == "zero":
        return np.zeros((40, 40))
    raise ValueError(name)


EIGH_NAMES = ["dead200", "dup200", "both200", "both600", "diag0", "rank1", "cI", "zero"]
EIGH_CASES = {}
for _name in EIGH_NAMES:
    EIGH_CASES[_name] = _eigh_case(_name)
    EIGH_CASES[_name].setflags(write=False)


def check_eigh(name, H, w, Vh):
    """The eigensolver bars on (w ascending, Vh rows = eigenvectors of the
    descending eigenvalues), as test_gpu_solver.py::test_eigh with the bar for
    exactly repeated eigenvalues (the null space is one).  Returns the figures."""
    n = H.shape[0]
    assert np.isfinite(w).all() and np.isfinite(Vh).all(), name
    orth = float(np.abs(Vh @ Vh.T - np.eye(n)).max())
    if name == "zero":
        wmax = float(np.abs(w).max())
        assert wmax <= 1e-290, (name, wmax)
        assert orth <= 1e-10, (name, orth)
        return dict(eig=wmax, resid=0.0, orth=orth)
    L = np.linalg.eigvalsh(H)
    nrm = max(np.abs(L).max(), 1e-300)
    eig = float(np.max(np.abs(w - L)) / nrm)
    lam = w[::-1]
    resid = float(np.linalg.norm(Vh @ H - lam[:, None] * Vh, axis=1).max() / nrm)
    assert eig <= 1e-12 * max(1, np.sqrt(n) / 8), (name, eig)
    assert resid <= 1e-9, (name, resid)
    assert orth <= 1e-10, (name, orth)
    return dict(eig=eig, resid=resid, orth=orth)


# ---------------------------------------------------------------------------
# pivot-stage cases: (n, dead, pairs), k = structural rank
# ---------------------------------------------------------------------------
PIVOT_CASES = [(200, 7, 0), (200, 7, 5), (1280, 40, 24)]


@functools.lru_cache(maxsize=None)
def pivot_case(case):
    """-> (H, k, order, Rx_ref, dead, pairs) with the order and factor of
    test_complement_math.pivoted_cholesky; computed once, read-only."""
    from test_complement_math import pivoted_cholesky
    n, nd, npair = case
    X, dead, pairs = degenerate_x(3 * n // 2, n, nd, npair, 7 * n + nd + npair)
    H = hessian(X, pairs)
    k = structural_rank(n, dead, pairs)
    order, Rx_ref = pivoted_cholesky(H, k)
    for a in (H, order, Rx_ref, dead):
        a.setflags(write=False)
    return H, k, order, Rx_ref, dead, tuple(pairs)


# ---------------------------------------------------------------------------
# whole-pipeline cases
# ---------------------------------------------------------------------------
# (n, m, n_dead, n_pairs, bits, group, sym, rule, threshold)
PIPE_CASES = [
    (200, 24, 7, 5, 4, -1, False, "energy", 1e-9),
    (384, 48, 13, 9, 4, 128, False, "energy", 1e-9),
    (384, 48, 13, 9, 3, 128, True, "mean_trimmed", 5e-4),   # the default rule and threshold
]
PIPE_IDS = ["n200-w4a-energy", "n384-w4a-g128-energy", "n384-w3s-g128-mt"]
PIPE_BLOCK = 128


@functools.lru_cache(maxsize=None)
def pipe_inputs(case):
    """-> (X fp16 (3n/2 x n), dead, pairs, W float32 (m x n)); the two n = 384
    cases share X and W."""
    n, m, nd, npair = case[:4]
    X, dead, pairs = degenerate_x(3 * n // 2, n, nd, npair, 1000 + n)
    W = (np.random.default_rng(2000 + n).standard_normal((m, n)) * 0.05).astype(F32)
    for a in (X, dead, W):
        a.setflags(write=False)
    return X, dead, tuple(pairs), W
