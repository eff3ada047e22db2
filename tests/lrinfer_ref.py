"""Host references and the shared case data of the low-rank inference tests
(test_gpu_lrinfer.py; checked without a GPU in test_lrinfer_ref.py).

  Z = X B^T                          tg_lr_down
  Y = round(Y32 + Z A^T + bias)      tg_lr_finish

The exact data: X, B and A hold small integers, Y32 multiples of 2^-6 and the
bias multiples of 2^-4 (exact in bf16).  With everything scaled by 64 each term
is an integer; while the sum of the *absolute* terms stays below 2^24 every
partial sum of every summation order is exact in fp32, so the kernels must reproduce Z bit for bit and Y as the
one rounding of the exact value.  Y32 is planted with +-70000 (beyond fp16's
65504: the fp16 output must be +-inf) and is mostly inexact in fp16 and bf16
(multiples of 2^-6 up to 4096), so the single rounding is observable.

`down_splits` restates the split heuristic of tg_lr_down; the CPU test checks
it against tg_lr_down_workspace_size, and with it the two shapes that were
chosen as the smallest n at which each regime splits K.
"""
import functools

import numpy as np
import torch

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
M = 104                                   # a full 64-feature tile and a partial one
NS = [32, 160, 488, 520, 1024]            # 488 / 520: the first n with two splits (mfma / gemv)
TS = [1, 4, 5, 17, 40, 130]
RS = [1, 8, 33, 64, 128]
HOT = 70000.0                             # exact in fp32, beyond fp16

# dispatch constants of lrinfer.hip
TARGET_WGS, GD_WAVES, GD_PASS, GD_MAX_T = 512, 4, 512, 16
MD_BM, MD_BN, MD_TK, MD_MIN_SLABS = 128, 32, 32, 8


def cdiv(a, b):
    return -(-a // b)


def gemv_splits(r, n):
    passes, tiles = cdiv(n, GD_PASS), cdiv(r, GD_WAVES)
    S = max(1, min(cdiv(TARGET_WGS, tiles), passes))
    return cdiv(n, cdiv(passes, S) * GD_PASS)


def mfma_splits(T, r, n):
    nslab = cdiv(n, MD_TK)
    tiles = cdiv(r, MD_BN) * cdiv(T, MD_BM)
    S = max(1, min(cdiv(TARGET_WGS, tiles), max(1, nslab // MD_MIN_SLABS)))
    return cdiv(nslab, cdiv(nslab, S))


def down_splits(T, r, n, regime):
    return gemv_splits(r, n) if regime == "gemv" else mfma_splits(T, r, n)


def workspace_bytes(T, r, n):
    S = mfma_splits(T, r, n)
    if T <= GD_MAX_T:
        S = max(S, gemv_splits(r, n))
    return 0 if S <= 1 else S * T * r * 4 + 256


def regimes(T):
    return ["gemv", "mfma"] if T <= GD_MAX_T else ["mfma"]


def dtypes_for(i):
    """A rotation through the operand types so the shape sweep sees them all."""
    x = ("f16", "bf16")[i % 2]
    b = ("f16", "bf16", "f32")[(i // 2) % 3]
    a = ("bf16", "f32", "f16")[(i // 3) % 3]
    bias = (None, "f16", "f32", "bf16")[(i // 5) % 4]
    y = ("f16", "f32", "bf16")[(i // 7) % 3]
    return x, b, a, bias, y


@functools.lru_cache(maxsize=None)
def exact_case(T, n, r, m=M):
    """Integer data (float64 arrays holding the exact values) and the exact
    results: X (T, n), B (r, n), A (m, r), Y32 (T, m), bias (m,), Z = X B^T,
    and y64 = Y32 + Z A^T + bias, with the largest scaled absolute sums."""
    rng = np.random.default_rng(7000 + 131 * T + 17 * n + r)
    X = rng.integers(-3, 4, size=(T, n)).astype(np.float64)
    B = rng.integers(-3, 4, size=(r, n)).astype(np.float64)
    A = rng.integers(-2, 3, size=(m, r)).astype(np.float64)
    Y32 = rng.integers(-4096 * 64, 4096 * 64 + 1, size=(T, m)).astype(np.float64) / 64
    Y32[0, 0], Y32[T - 1, m - 1] = HOT, -HOT
    if T > 1:
        Y32[T // 2, m // 2] = HOT
    bias = rng.integers(-8 * 16, 8 * 16 + 1, size=m).astype(np.float64) / 16    # exact in bf16
    Z = X @ B.T
    y_nb = Y32 + Z @ A.T
    abs_z = float((np.abs(X) @ np.abs(B).T).max())
    abs_y = float(((np.abs(Y32) + np.abs(Z) @ np.abs(A).T + np.abs(bias)) * 64).max())
    out = dict(X=X, B=B, A=A, Y32=Y32, bias=bias, Z=Z, y_nobias=y_nb, y_bias=y_nb + bias,
               abs_z=abs_z, abs_y=abs_y)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def as_tensor(a, dt):
    """The float64 image as a CPU tensor of type dt (exact for the data above)."""
    t = torch.from_numpy(np.array(a)).to(TDT[dt])
    assert torch.equal(t.double(), torch.from_numpy(np.array(a)))
    return t


def rounded(y64, dt):
    """The one rounding of the exact result: float64 -> float32 is exact here."""
    y32 = torch.from_numpy(np.array(y64)).to(torch.float32)
    assert torch.equal(y32.double(), torch.from_numpy(np.array(y64)))
    return y32.to(TDT[dt])


def raw_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def ulp(y64, dt):
    """Spacing of dt at |y64|."""
    a = np.abs(y64)
    e = np.floor(np.log2(np.maximum(a, 1e-300)))
    if dt == "f16":
        return 2.0 ** (np.maximum(e, -14) - 10)
    if dt == "bf16":
        return 2.0 ** (np.maximum(e, -126) - 7)
    return 2.0 ** (np.maximum(e, -126) - 23)
