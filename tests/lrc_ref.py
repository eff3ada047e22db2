"""Host restatement of the low-rank correction (tg_lrc_factor) in numpy float64,
and the inputs shared by test_lrc_ref.py (CPU) and test_gpu_lrc.py.

The correction of a residual E (m x n) under tr((E - A B) H (E - A B)^T) is the
truncated SVD of G = E H^(1/2) mapped back: A B = Q Q^T E with Q the top-r left
singular vectors of G; the error that is left is the tail sum of the squared
singular values mu_i (Eckart-Young).  `svd_route` computes exactly that.
`gram_route` and `factor_route` restate the three routes of the library (the
eigenproblem of E H E^T, of M M^T and of M^T M with M = E F^T) with
numpy.linalg.eigh, so the CPU test can show that they agree with the SVD route
before any GPU result is compared with it.
"""
import functools

import numpy as np

EPS = 2.0 ** -52


def sqrt_psd(H):
    """H^(1/2) of a symmetric positive semi-definite H (eigenvalues clamped at 0)."""
    lam, V = np.linalg.eigh(0.5 * (H + H.T))
    return (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T


def kept_rank(mu, n):
    """Number of leading directions with mu_j > n 2^-52 mu_1."""
    mu = np.asarray(mu, dtype=np.float64)
    if mu.size == 0 or not mu[0] > 0.0:
        return 0
    return int(np.count_nonzero(mu > n * EPS * mu[0]))


def finish(E, Q, mu_all, r):
    """(A0, B0, dict) from orthonormal Q (m x >= r, descending) and the whole
    descending spectrum mu_all: directions past the kept rank are zeroed."""
    m, n = E.shape
    mu = np.zeros(r)
    top = np.asarray(mu_all[:r], dtype=np.float64)
    k = kept_rank(top, n)
    mu[:k] = top[:k]
    A0 = np.zeros((m, r))
    A0[:, :k] = Q[:, :k]
    B0 = A0.T @ E
    err0 = float(np.sum(mu_all))
    return A0, B0, dict(mu=mu, err0=err0, err1=err0 - float(mu.sum()), rank=k,
                        tail=float(np.sum(mu_all[r:])))


def svd_route(E, H, r):
    G = E @ sqrt_psd(H)
    U, s, _ = np.linalg.svd(G, full_matrices=False)
    return finish(E, U, s * s, r)


def _eigh_desc(K):
    lam, V = np.linalg.eigh(0.5 * (K + K.T))
    return lam[::-1], V[:, ::-1]


def gram_route(E, H, r):
    """gram = 1: the top eigenvectors of K = (E H) E^T."""
    lam, V = _eigh_desc((E @ H) @ E.T)
    return finish(E, V, np.maximum(lam, 0.0), r)


def factor_route(E, F, r):
    """gram = 0, F (p x n) with H = F^T F: the m-route (m <= p) or the p-route."""
    m, p = E.shape[0], F.shape[0]
    M = E @ F.T
    if m <= p:
        lam, V = _eigh_desc(M @ M.T)
        return finish(E, V, np.maximum(lam, 0.0), r)
    lam, P = _eigh_desc(M.T @ M)
    lam = np.maximum(lam, 0.0)
    re = min(r, p)
    k = kept_rank(lam[:re], E.shape[1])
    Q = np.zeros((m, r))
    Q[:, :k] = (M @ P[:, :k]) / np.sqrt(lam[:k])
    return finish(E, Q, lam, r)


def balance(A0, B0):
    """A = A0 s, B = B0 / s with s_j = 2^rint(log2(max|B0_j| / max|A0_j|) / 2)."""
    A, B = A0.copy(), B0.copy()
    for j in range(A0.shape[1]):
        ma, mb = np.abs(A0[:, j]).max(), np.abs(B0[j]).max()
        if not (ma > 0.0 and mb > 0.0):
            A[:, j] = 0.0
            B[j] = 0.0
            continue
        e = int(np.clip(np.rint(0.5 * np.log2(mb / ma)), -1000, 1000))
        A[:, j] = np.ldexp(A0[:, j], e)
        B[j] = np.ldexp(B0[j], -e)
    return A, B


def unbalance(A):
    """A0 from a balanced A: a unit column times 2^e has norm 2^e."""
    A0 = np.zeros_like(A, dtype=np.float64)
    for j in range(A.shape[1]):
        nrm = np.linalg.norm(A[:, j])
        if nrm > 0.0:
            A0[:, j] = np.ldexp(A[:, j], -int(np.rint(np.log2(nrm))))
    return A0


def weighted_error(E, AB, H):
    """tr((E - AB) H (E - AB)^T), evaluated directly."""
    D = E - AB
    return float(np.sum((D @ H) * D))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def dense_h(n, seed):
    """A well conditioned H = X^T X / N from N = 3n Gaussian rows."""
    X = np.random.default_rng(seed).standard_normal((3 * n, n))
    H = X.T @ X / X.shape[0]
    return 0.5 * (H + H.T)


def conditioned_factor(p, n, rng):
    """F (p x n, p <= n) with singular values from 2 down to 1/2, so that
    H = F^T F has rank p and its non-zero eigenvalues lie in [1/4, 4]."""
    left = np.linalg.qr(rng.standard_normal((p, p)))[0]
    right = np.linalg.qr(rng.standard_normal((n, n)))[0][:, :p]
    return (left * np.linspace(2.0, 0.5, p)) @ right.T


def degenerate_h(n, n_dead, n_pairs, seed):
    """H with exactly zero rows / columns (dead channels) and exactly repeated
    ones (duplicated channels), as tests/degenerate_ref.py builds them."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, n))
    p = rng.permutation(n)
    dead = np.sort(p[:n_dead])
    rest = p[n_dead:n_dead + 2 * n_pairs]
    pairs = [(int(rest[2 * i]), int(rest[2 * i + 1])) for i in range(n_pairs)]
    for a, b in pairs:
        X[:, b] = X[:, a]
    X[:, dead] = 0.0
    H = X.T @ X / X.shape[0]
    H = 0.5 * (H + H.T)
    for a, b in pairs:
        H[b, :] = H[a, :]
        H[:, b] = H[:, a]
    return H, dead, pairs


def residual_with_gap(m, H, r, seed, rank=None):
    """E (float32, m x n) = sum_j sigma_j u_j v_j^T H^(-1/2) (the pseudo-inverse
    root on H's range) plus a part in H's null space that the objective does
    not see.  sigma_1 .. sigma_r fall from 2 to 1 and the noise directions
    sigma_{r+1} .. lie in [1/8, 1/4], so mu_r / mu_{r+1} >= 16 before the
    rounding of E to float32 (which moves it by ~1e-7).  `rank` limits the
    number of non-zero directions (no noise then)."""
    rng = np.random.default_rng(seed)
    n = H.shape[0]
    lam, V = np.linalg.eigh(H)
    pos = lam > 1e-10 * lam[-1]
    Vp, lp = V[:, pos], lam[pos]
    t = min(m, Vp.shape[1])
    U = np.linalg.qr(rng.standard_normal((m, t)))[0]
    C = np.linalg.qr(rng.standard_normal((Vp.shape[1], t)))[0]
    sig = np.empty(t)
    top = min(r, t)
    sig[:top] = np.linspace(2.0, 1.0, top) if top > 1 else 2.0
    sig[top:] = rng.uniform(0.125, 0.25, t - top)
    if rank is not None:
        sig[rank:] = 0.0
    E = (U * sig) @ C.T @ (Vp / np.sqrt(lp)).T
    if Vp.shape[1] < n:                                  # unseen by H
        Vn = V[:, ~pos]
        E = E + 0.3 * rng.standard_normal((m, Vn.shape[1])) @ Vn.T
    return E.astype(np.float32)


# (name, m, n, kind, p): kind "gram" passes H itself; "factor" passes F (p x n,
# float64) through a non-trivial perm; "sketch" passes a float32 F without perm.
SHAPES = [
    ("gram-48x96", 48, 96, "gram", None),
    ("factor-48x96-p80", 48, 96, "factor", 80),          # m <= p: the m-route
    ("factor-160x64-p64", 160, 64, "factor", 64),        # m > p: the p-route
    ("gram-24x160", 24, 160, "gram", None),
    ("factor-24x160-p160", 24, 160, "factor", 160),
    ("gram-320x96", 320, 96, "gram", None),              # an eigenproblem of order 320
    ("factor-320x96-p96", 320, 96, "factor", 96),
]
RANKS = [1, 4, 16]
CASES = [(s, r) for s in SHAPES for r in RANKS] + [
    (("gram-320x128", 320, 128, "gram", None), 100),
    (("factor-320x128-p128", 320, 128, "factor", 128), 100),
]
CASE_IDS = [f"{s[0]}-r{r}" for s, r in CASES]


@functools.lru_cache(maxsize=None)
def _case(name, m, n, kind, p, r):
    seed = sum(ord(c) for c in name) * 131 + r
    rng = np.random.default_rng(seed)
    if kind == "gram":
        H = dense_h(n, seed + 1)
        F = perm = None
    else:
        F = conditioned_factor(p, n, rng)
        H = F.T @ F
        perm = rng.permutation(n).astype(np.int64)
    E = residual_with_gap(m, H, r, seed + 2)
    out = dict(E=E, H=H, F=F, perm=perm, r=r, kind=kind)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def case(shape, r):
    """The inputs of one entry of CASES (cached, read-only): E float32, H
    float64, and for the factor kinds F with H = F^T F and perm; the library is
    given Rx = F[:, perm], so that Rx[:, j] = F[:, perm[j]]."""
    return _case(*shape, r)


def reference(c):
    """svd_route on the float64 image of the case's E."""
    return svd_route(c["E"].astype(np.float64), c["H"], c["r"])


@functools.lru_cache(maxsize=None)
def rank3_case():
    H = dense_h(96, 901)
    E = residual_with_gap(48, H, 8, 902, rank=3)
    E.setflags(write=False)
    H.setflags(write=False)
    return dict(E=E, H=H, F=None, perm=None, r=8, kind="gram")


@functools.lru_cache(maxsize=None)
def degenerate_case():
    H, dead, pairs = degenerate_h(96, 5, 4, 911)
    E = residual_with_gap(48, H, 8, 912)
    E.setflags(write=False)
    H.setflags(write=False)
    return dict(E=E, H=H, F=None, perm=None, r=8, kind="gram", dead=dead, pairs=pairs)


@functools.lru_cache(maxsize=None)
def sketch_case():
    """A float32 sketch Y (p x n) as factor, against gram = 1 with H = Y^T Y."""
    rng = np.random.default_rng(921)
    Y = (rng.standard_normal((128, 96)) / np.sqrt(128)).astype(np.float32)
    Y64 = Y.astype(np.float64)
    H = Y64.T @ Y64
    E = residual_with_gap(48, H, 8, 922)
    for a in (Y, H, E):
        a.setflags(write=False)
    return dict(E=E, H=H, F=Y, perm=None, r=8, kind="sketch")
