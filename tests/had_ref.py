"""Host reference of the Hadamard rotation (A18) for test_gpu_hadamard.py,
test_gpu_had_solver.py and test_gpu_had_model.py; proved on the CPU in
test_had_ref.py.  Plain numpy restatement of the contract in
include/truncgptq.h: every operation of the compute type is one numpy operation
of that type, in the order the contract writes it.

  pack_signs / unpack_signs   s in {+1, -1}^n <-> int32 words, bit j of word i =
                              column 32 i + j is negated
  butterflies   stages h = 1, 2, ... b/2 inside each block of b columns
  rows          R(x) = x Q and R^-1(y) = y Q^T on the last axis; f64 computes in
                f64, everything else in f32; one rounding to the output type
  sym           Q^T H Q in f64: rows, then the same operator along the row index,
                the upper triangle overwritten by the mirror of the lower one
  q_matrix      Q as an explicit float64 matrix (kron of Sylvester matrices)
"""
import numpy as np
import torch

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
BLOCKS = [32, 64, 128, 256, 512, 1024, 2048, 4096]
ROWS = [1, 3, 17, 65]
# (input, output): every pair the f32 compute type takes, and f64 -> f64
DTYPE_PAIRS = [(a, b) for a in ("f16", "bf16", "f32") for b in ("f16", "bf16", "f32")] \
    + [("f64", "f64")]
SYM_CASES = [(32, 32), (96, 32), (768, 32), (768, 256), (4096, 32), (4096, 256), (4096, 4096)]


def pack_signs(s):
    """int32 words of a vector of +1 / -1 (length a multiple of 32)."""
    s = np.asarray(s)
    assert s.ndim == 1 and s.size % 32 == 0 and np.all(np.abs(s) == 1)
    bits = (s < 0).reshape(-1, 32).astype(np.uint64)
    words = (bits << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    return words.view(np.int32)


def unpack_signs(words, n):
    """float64 +1 / -1 of n columns; None = all +."""
    if words is None:
        return np.ones(n)
    w = np.asarray(words, dtype=np.int32).view(np.uint32)
    assert w.shape == (n // 32,)
    bits = (w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
    return np.where(bits.reshape(-1) == 1, -1.0, 1.0)


def random_signs(n, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)


def mixed_signs(n, b, seed=0):
    """Both signs inside every word, and blocks that differ from each other."""
    s = random_signs(n, seed)
    s[0::32], s[1::32] = 1.0, -1.0
    for k in range(n // b):
        s[k * b + 2] = -1.0 if k % 2 else 1.0
    return s


def butterflies(v, b):
    """The stages on the last axis of v (a multiple of b wide), in v's dtype."""
    shape = v.shape
    v = v.reshape(-1, shape[-1] // b, b).copy()
    h = 1
    while h < b:
        w = v.reshape(v.shape[0], v.shape[1], b // (2 * h), 2, h)
        u, x = w[:, :, :, 0, :], w[:, :, :, 1, :]
        d = u - x
        u += x
        x[...] = d
        h *= 2
    return v.reshape(shape)


def scale_of(b, ct):
    c = 1.0 / np.sqrt(np.float64(b))
    return np.float32(c) if ct == np.float32 else np.float64(c)


def rows_np(x, b, words=None, inverse=False):
    """The operator in x's dtype (float32 or float64), before the output rounding."""
    ct = x.dtype.type
    assert ct in (np.float32, np.float64)
    n = x.shape[-1]
    assert b >= 32 and b & (b - 1) == 0 and n % b == 0
    s = unpack_signs(words, n).astype(ct)
    v = x if inverse else x * s
    v = butterflies(np.ascontiguousarray(v), b) * scale_of(b, ct)
    return v * s if inverse else v


def rows(x, b, words=None, inverse=False, out=None):
    """x: a CPU tensor (f16 / bf16 / f32 / f64) -> a CPU tensor of type `out`
    (a TDT key; default: x's type)."""
    odt = x.dtype if out is None else TDT[out]
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    assert (odt == torch.float64) == (x.dtype == torch.float64)
    y = rows_np(x.to(ct).numpy(), b, words, inverse)
    return torch.from_numpy(y).to(odt)


def sym(H, b, words=None):
    """Q^T H Q of a float64 matrix, exactly symmetric."""
    H = np.asarray(H, dtype=np.float64)
    P = rows_np(H, b, words)
    P = np.ascontiguousarray(rows_np(np.ascontiguousarray(P.T), b, words).T)
    return np.tril(P) + np.tril(P, -1).T


def sylvester(b):
    Hm = np.ones((1, 1))
    while Hm.shape[0] < b:
        Hm = np.block([[Hm, Hm], [Hm, -Hm]])
    return Hm


def q_matrix(n, b, words=None):
    """Q = diag(s) (I (x) H_b) / sqrt(b), float64."""
    return unpack_signs(words, n)[:, None] * np.kron(np.eye(n // b), sylvester(b)) / np.sqrt(b)


def raw_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def integer_rows(rows_, n, seed):
    """Integers with |x| <= 8 (float64): every stage and the output are exact in
    every type while b |x| stays below the type's integer range."""
    return np.random.default_rng(seed).integers(-8, 9, (rows_, n)).astype(np.float64)


# ---------------------------------------------------------------------------
# the quality case of the issue
# ---------------------------------------------------------------------------
def outlier_weight(m, n, seed, cols=4, factor=30.0):
    """W = 0.02 N(0, 1) with `cols` columns multiplied by `factor` (float32)."""
    rng = np.random.default_rng(seed)
    W = 0.02 * rng.standard_normal((m, n))
    W[:, rng.choice(n, cols, replace=False)] *= factor
    return W.astype(np.float32)


def weighted_error(W, Wq, H):
    """tr((W - Wq) H (W - Wq)^T) in float64."""
    E = np.asarray(W, dtype=np.float64) - np.asarray(Wq, dtype=np.float64)
    return float(np.einsum("ij,jk,ik->", E, np.asarray(H, dtype=np.float64), E))


QUALITY = dict(m=32, n=256, b=128, bits=4, group=128, seed=0, sign_seed=7)


def quality_case():
    """(W f32, H f64, sign words) of the one quality condition."""
    from mx_ref import hessian_case
    q = QUALITY
    W = outlier_weight(q["m"], q["n"], q["seed"])
    H = hessian_case(q["n"], 4 * q["n"], q["seed"])
    return W, H, pack_signs(random_signs(q["n"], q["sign_seed"]))
