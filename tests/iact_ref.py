"""Host restatement of INT8 activations (A20): the per-token quantiser of
tg_quant_act_i8 operation by operation in float32, and D and Y of tg_qgemm_act
with D exact (int64) and everything after it in float64.  The weights come from
the oracle's packer, like qlinear_ref.packed_case."""
import functools

import numpy as np

from qlinear_ref import oracle

F32 = np.float32


def quantize(x, g):
    """x: CPU torch tensor (T, n), fp16 / bf16 -> (q int8 (T, n), xs f32 (T,),
    xsum int32 (T, n / g))."""
    x32 = x.float().numpy()
    T, n = x32.shape
    xs = np.abs(x32).max(axis=1) / F32(127)
    assert xs.dtype == F32
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint(x32 / xs[:, None])                    # float32 division, ties to even
    q = np.where(xs[:, None] > 0, np.clip(r, -127, 127), 0).astype(np.int64)
    return q.astype(np.int8), xs, q.reshape(T, n // g, g).sum(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def weights(m, n, g, b, kind):
    """Random unsigned codes (m, n), zeros and scales (m, G), and the packed
    triple.  kind "pow2": scales 2^-6 .. 2^-2; "small": W^ ~ O(0.05).  Rows 0 and
    1 hold both extremes: code 0 against zero 2^b - 1, and the reverse."""
    g = g if g > 0 else n
    rng = np.random.default_rng(100 * b + m + n + g)
    top = 2 ** b - 1
    codes = rng.integers(0, top + 1, size=(m, n))
    zero = rng.integers(0, top + 1, size=(m, n // g))
    codes[0, :8], zero[0] = 0, top
    codes[1, :8], zero[1] = top, 0
    if kind == "pow2":
        scale = (2.0 ** rng.integers(-6, -1, size=zero.shape)).astype(F32)
    else:
        scale = (rng.uniform(0.05, 0.1, size=zero.shape) / 2 ** (b - 1)).astype(F32)
    return (codes, zero, scale) + tuple(oracle().pack_weights(codes, scale, zero.astype(F32), b,
                                                              False))


def gemm(q, xs, codes, zero, scale, g, b, bias=None):
    """-> (y64, mag): Y of the contract in float64 on exact D, and xs sum_j |D|
    scale + |bias|, the magnitude its error bound multiplies."""
    off = 128 if b == 8 else 0
    (T, n), m = q.shape, codes.shape[0]
    g = g if g > 0 else n
    qg = q.astype(np.int64).reshape(T, n // g, g)
    D = np.einsum("tjk,rjk->tjr", qg, (codes - off).reshape(m, n // g, g)) \
        - (zero - off).T[None] * qg.sum(-1)[:, :, None]
    assert np.abs(D).max() < 2 ** 31
    s = scale.T.astype(np.float64)[None]
    xs = xs.astype(np.float64)[:, None]
    y, mag = xs * (D * s).sum(1), xs * (np.abs(D) * s).sum(1)
    if bias is not None:
        y, mag = y + bias.astype(np.float64)[None], mag + np.abs(bias).astype(np.float64)[None]
    return y, mag
