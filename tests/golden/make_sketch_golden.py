"""Generate the sketch-mode golden vectors by running the REFERENCE's own
``Sketcher`` and ``process_sketch`` on the CPU (same shim as make_golden.py:
``jax.scipy.linalg.qr(pivoting=True)`` -> LAPACK dgeqp3 through scipy).

Runs only where the reference checkout exists (the build container).  The
fixtures hold data only: the fp32 sketch Y the reference accumulated from
``synth.make_x`` inputs, and what its ``process_sketch`` returned for it
(R float64, perm, k).  Each case is written as ``k_<case>_p<i>.npz`` parts of
less than 1 MB (arrays are cut into row blocks ``<key>__<j>``);
``load_sketch_golden`` below puts a case together again and is what the tests
import.

    python tests/golden/make_sketch_golden.py [case names]
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900_000

# name, xkind, n, rank, tokens, eps, method, seed
CASES = [
    ("k_ar1_n256_r512_mt", "ar1", 256, 512, 2048, 1e-2, "mean_trimmed", 11),
    ("k_logn_n256_r1024_e4", "lognormal", 256, 1024, 1024, 1e-4, "energy", 12),
    ("k_ar1_n512_r512_t300_e4", "ar1", 512, 512, 300, 1e-4, "energy", 13),
    # mean_trimmed with directions truncated: 150 tokens, so S[150:] is the fp32
    # sketch's rounding level (1.7e-7) under the threshold 1e-2 S[1:33].mean() =
    # 2.3e-2, and k = 150
    ("k_ar1_n256_r256_t150_mt", "ar1", 256, 256, 150, 1e-2, "mean_trimmed", 14),
]


def sketch_golden_names():
    return sorted({os.path.basename(f).rsplit("_p", 1)[0]
                   for f in glob.glob(os.path.join(HERE, "k_*_p*.npz"))})


def load_sketch_golden(name):
    chunks = {}
    for f in sorted(glob.glob(os.path.join(HERE, name + "_p*.npz"))):
        with np.load(f, allow_pickle=False) as z:
            for key in z.files:
                base, j = key.rsplit("__", 1)
                chunks.setdefault(base, {})[int(j)] = z[key]
    out = {}
    for base, parts in chunks.items():
        arrs = [parts[j] for j in sorted(parts)]
        out[base] = arrs[0] if arrs[0].ndim == 0 else np.concatenate(arrs, axis=0)
    return out


def save_parts(name, arrays):
    for f in glob.glob(os.path.join(HERE, name + "_p*.npz")):
        os.remove(f)
    pieces = []
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.ndim == 0 or a.nbytes <= PART_BYTES // 2:
            pieces.append((f"{key}__0", a))
            continue
        rows = max(1, (PART_BYTES // 2) // (a.nbytes // a.shape[0]))
        for j, r0 in enumerate(range(0, a.shape[0], rows)):
            pieces.append((f"{key}__{j}", a[r0:r0 + rows]))
    files, cur, size = [], {}, 0
    for key, a in pieces:
        if cur and size + a.nbytes > PART_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[key] = a
        size += a.nbytes
    files.append(cur)
    for i, d in enumerate(files):
        path = os.path.join(HERE, f"{name}_p{i}.npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    return len(files)


def pivot_gaps(Y, k, perm):
    """The greedy column pivoting of diag(S_k) Vh_k (what dgeqp3 does), redone
    in float64: every chosen pivot must be `perm`'s and beat the runner-up
    remaining column norm by more than 1e-6 relative, so that an identical
    perm is a fair demand of any correct implementation."""
    _, S, Vh = np.linalg.svd(Y.astype(np.float64), full_matrices=False)
    A = S[:k, None] * Vh[:k]
    free = np.ones(A.shape[1], dtype=bool)
    worst = np.inf
    for i in range(k):
        norms = np.where(free, np.linalg.norm(A, axis=0), -1.0)
        order = np.argsort(norms)
        p, second = order[-1], order[-2]
        assert p == perm[i], (i, p, perm[i])
        gap = (norms[p] - norms[second]) / norms[p]
        assert gap > 1e-6, f"pivot {i}: gap {gap:.2e}; change the seed"
        worst = min(worst, gap)
        q = A[:, p] / norms[p]
        A -= np.outer(q, q @ A)
        free[p] = False
    return worst


def gen_case(g, torch, make_x, spec):
    name, xkind, n, rank, tokens, eps, method, seed = spec
    gen = torch.Generator().manual_seed(seed)
    X = make_x(xkind, tokens, n, gen)
    torch.manual_seed(seed)                      # the reference draws Omega from the global generator
    sk = g.Sketcher(torch.nn.Linear(n, 8), rank, device="cpu")
    h = tokens // 3                              # three hook calls, one of them 3-D
    sk.hook_fn(None, (X[:h].reshape(1, h, n),), None)
    sk.hook_fn(None, (X[h:2 * h],), None)
    sk.hook_fn(None, (X[2 * h:],), None)
    assert sk.n_samples == tokens
    Y = sk.get_scaled_sketch().clone()
    R, perm = g.process_sketch(Y.clone(), threshold=eps, threshold_method=method)
    k = R.shape[0]
    Yn, permn = Y.numpy(), perm.numpy().astype(np.int64)
    worst = pivot_gaps(Yn, k, permn)
    nf = save_parts(name, dict(Y=Yn, R=R.numpy(), perm=permn, k=np.int64(k), eps=np.float64(eps),
                               method=np.str_(method), tokens=np.int64(tokens)))
    print(f"{name}: n={n} rank={rank} tokens={tokens} k={k} smallest pivot gap {worst:.2e} "
          f"({nf} parts)")


def main():
    sys.path.insert(0, HERE)
    import torch
    from make_golden import install_shim
    from synth import make_x
    g = install_shim()
    only = set(sys.argv[1:])           # case names; none = all
    for spec in CASES:
        if not only or spec[0] in only:
            gen_case(g, torch, make_x, spec)


if __name__ == "__main__":
    main()
