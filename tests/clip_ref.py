"""numpy restatement of the clip search's contract (include/truncgptq.h,
tg_group_params_clip) and the inputs its tests share (test_clip_host.py,
test_gpu_clip.py).

Every f32 operation is one numpy float32 operation in the order the contract
writes it; the objective is summed in float64 (numpy's pairwise sum -- the
contract leaves the order to the implementation).  `clip_search` returns every
candidate's (s, z, J) and the choice: the smallest i with minimal J_i.
"""
import functools

import numpy as np

F32 = np.float32

# (m, n, group) of the parity tests; the last two stream a per-row group
SHAPES = [(37, 330, -1), (37, 330, 110), (5, 384, 128), (7, 256, 32), (3, 96, 16), (3, 64, 1),
          (2, 8256, -1), (2, 28672, -1)]
BITS = [2, 3, 4, 8]
GRID, STEPS = 100, 80


def qrange(bits, sym):
    if sym:
        h = 2 ** (bits - 1) - 1
        return -h, h
    return 0, 2 ** bits - 1


def clip_search(W, h, bits, group, sym, grid=GRID, steps=STEPS):
    """-> dict(s, z: (m, G, C) f32; J: (m, G, C) f64; choice: (m, G) int32)."""
    W = np.ascontiguousarray(W, dtype=F32)
    m, n = W.shape
    g = group if group > 0 else n
    assert n % g == 0 and grid >= 1 and 0 <= steps < grid
    G, C = n // g, steps + 1
    minq, maxq = (F32(v) for v in qrange(bits, sym))
    w = W.reshape(m, G, g)
    hd = (np.ones(n) if h is None else np.asarray(h, dtype=F32).astype(np.float64)).reshape(G, g)
    s = np.empty((m, G, C), dtype=F32)
    z = np.empty((m, G, C), dtype=F32)
    J = np.empty((m, G, C), dtype=np.float64)
    if sym:
        a = np.max(np.abs(w), axis=2)
    else:
        mn, mx = np.min(w, axis=2), np.max(w, axis=2)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(C):
            p = F32(1.0) - F32(i) / F32(grid)
            if sym:
                si = (np.maximum(p * a, F32(1e-5)) / maxq).astype(F32)
                zi = np.zeros_like(si)
            else:
                lo = np.where(mn < 0, p * mn, mn).astype(F32)
                hi = np.where(mx > 0, p * mx, mx).astype(F32)
                si = (np.maximum(hi - lo, F32(1e-5)) / maxq).astype(F32)
                zi = np.clip(np.rint(-lo / si), F32(0), maxq).astype(F32)
            sb, zb = si[:, :, None], zi[:, :, None]
            q = np.clip(np.rint(w / sb + zb), minq, maxq)
            dq = (q - zb) * sb
            e = (w - dq).astype(F32)
            assert q.dtype == F32 and dq.dtype == F32
            ed = e.astype(np.float64)
            J[:, :, i] = np.sum(hd[None] * (ed * ed), axis=2)
            s[:, :, i], z[:, :, i] = si, zi
    choice = np.argmin(J, axis=2).astype(np.int32)   # first index of the minimum
    return dict(s=s, z=z, J=J, choice=choice)


def ambiguous(ref):
    """(m, G) bool: the two lowest objectives are within 1e-9 relative, the
    lower is nonzero and the two candidates' (s, z) differ."""
    J, s, z = ref["J"], ref["s"], ref["z"]
    if J.shape[2] < 2:
        return np.zeros(J.shape[:2], dtype=bool)
    order = np.argsort(J, axis=2, kind="stable")
    i0, i1 = order[:, :, 0:1], order[:, :, 1:2]
    take = lambda a, i: np.take_along_axis(a, i, axis=2)[:, :, 0]
    j0, j1 = take(J, i0), take(J, i1)
    differ = (take(s, i0) != take(s, i1)) | (take(z, i0) != take(z, i1))
    return (j1 - j0 <= 1e-9 * j0) & (j0 != 0) & differ


def clip_input(m, n, group):
    """Student-t(4) * 0.02 weights with the eight degenerate group patterns of
    test_gpu_small_stages.group_params_input planted in the same positions."""
    rng = np.random.default_rng(m + n)
    W = (rng.standard_t(4, (m, n)) * 0.02).astype(F32)
    gg = n if group <= 0 else group
    G = n // gg
    patterns = [
        lambda k: np.full(k, 0.3),                                   # all equal
        lambda k: np.abs(rng.standard_normal(k)) + 0.01,             # all positive
        lambda k: -np.abs(rng.standard_normal(k)) - 0.01,            # all negative
        lambda k: 1.0 + 4e-6 * rng.random(k),                        # range under the clamp
        lambda k: np.where(np.arange(k) == k // 2, 1e20, rng.standard_normal(k)),  # outlier
        lambda k: np.zeros(k),                                       # +0
        lambda k: -np.zeros(k),                                      # -0
        lambda k: np.resize(np.array([0.0, -0.0, 0.5, -0.25]), k),   # signed zeros
    ]
    for i, pat in enumerate(patterns):
        r, gi = (i // G) % m, i % G
        W[r, gi * gg:(gi + 1) * gg] = pat(gg).astype(F32)
    return W


def clip_weights(n, bits):
    """lognormal(0, 1.5) column weights with every 7th entry 0 (dead channels)."""
    h = np.random.default_rng(n + bits).lognormal(0.0, 1.5, n).astype(F32)
    h[::7] = 0
    return h


def quality_problem(seed=11, n=256, m=64, tokens=2048, rho=0.9, sigma=1.0):
    """The end-to-end setting of DESIGN.md's clip-search experiment: AR(1)
    (rho) tokens with log-normal per-channel scales exp(normal(0, sigma)) and
    Student-t(4) weights; drawn in the order token noise, channel scales,
    weights.  -> (X tokens x n f64, W m x n f32)."""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((tokens, n))
    scales = np.exp(rng.normal(0.0, sigma, n))
    W = (rng.standard_t(4, (m, n)) * 0.02).astype(F32)
    idx = np.arange(n)
    L = np.linalg.cholesky(rho ** np.abs(idx[None, :] - idx[:, None]) + 1e-6 * np.eye(n))
    return (noise @ L.T) * scales[None, :], W


def proxy_error(W, Wq, X):
    """||(W - Wq) X^T||_F in float64."""
    D = np.asarray(W, dtype=np.float64) - np.asarray(Wq, dtype=np.float64)
    return float(np.linalg.norm(D @ np.asarray(X, dtype=np.float64).T))


@functools.lru_cache(maxsize=None)
def case(m, n, group, bits, sym, weighted):
    """(W, h or None, restatement), computed once per process and shared;
    callers leave the arrays unchanged."""
    W = clip_input(m, n, group)
    h = clip_weights(n, bits) if weighted else None
    ref = clip_search(W, h, bits, group, sym)
    for a in (W, h, *ref.values()):
        if a is not None:
            a.setflags(write=False)
    return W, h, ref
