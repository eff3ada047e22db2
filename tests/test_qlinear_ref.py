"""CPU: the host references of the packed-inference GPU tests (qlinear_ref.py)
and the shapes those tests rely on.

1. Every packed case decodes back to its codes and zeros through the oracle's
   unpacker, short last units and groups that are no multiple of 32 included.
2. Every exact GEMM case really is exact: the sum of the absolute terms of
   64 y (bias included) is below 2^24, so every partial sum of every summation
   order is an fp32 integer and the GPU comparison cannot be vacuous.  The
   16-bit output cases hold values that 16 bits cannot represent and, for fp16,
   values that overflow.
3. The wave-loop shapes still reach the wave loop: the workspace query gives
   the number of K splits S of the gemv regime, and 4 S < n / 32 means some
   wave of a workgroup owns more than one unit of 32 values.  Should the
   dispatch constants change, this fails instead of the GPU tests quietly no
   longer doing their job.
"""
import numpy as np
import pytest
import torch

import qlinear_ref as R


def case_id(c):
    return "-".join(str(v) for v in c)


# ---- 1. the packed words ----------------------------------------------------
def packed_keys():
    keys = {(c.m, c.n, c.g, c.b, "pow2") for c in R.EXACT_CASES}
    keys |= {(m, n, g, b, "rand") for m, n, g, b in R.DEQUANT_SHAPES}
    keys |= {(m, n, g, b, "pow2") for m, n, g, b in R.PACK_SHAPES}
    keys |= {(R.WAVE_M, R.WAVE_N, 128, b, "small") for b in (3, 4)}
    keys |= {(96, 1024, 128, 4, "small"), (96, 256, 128, 4, "small")}
    return sorted(keys)


def decodes(codes, zero, qw, qz, m, n, g, b):
    o = R.oracle()
    G = n // (g if g > 0 else n)
    assert qw.shape == (n * b // 32, m) and qz.shape == (G, m * b // 32)
    assert np.array_equal(o.unpack_rows_bitstream(qw, b, n).T, codes)
    assert np.array_equal(o.unpack_rows_bitstream(np.ascontiguousarray(qz.T), b, m), zero)


@pytest.mark.parametrize("key", packed_keys(), ids=lambda k: "-".join(map(str, k)))
def test_packed_words_decode(key):
    m, n, g, b, kind = key
    codes, zero, scale, qw, qz, sc = R.packed_case(m, n, g, b, kind)
    decodes(codes, zero, qw, qz, m, n, g, b)
    assert sc.shape == (zero.shape[1], m) and np.array_equal(sc.T, scale)
    # the top bit of the fields is exercised
    assert codes.min() < 2 ** (b - 1) <= codes.max()


@pytest.mark.parametrize("fill", ["max", "min"])
@pytest.mark.parametrize("shape", R.DEQUANT_FILL_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fill_words_decode_and_saturate(shape, fill):
    m, n, g, b = shape
    codes, zero, scale, qw, qz, sc = R.packed_fill(m, n, g, b, fill)
    decodes(codes, zero, qw, qz, m, n, g, b)
    sign = 1.0 if fill == "max" else -1.0
    w = sign * (2 ** b - 1) * 65504.0
    for out in ("f16", "bf16", "f32"):
        got = R.host_dequant(codes, zero, scale, g, out)
        want = torch.tensor(w, dtype=torch.float32).to(R.TDT[out])
        assert torch.all(got == want)
        assert bool(torch.isinf(want)) == (out == "f16")
    assert float(torch.tensor(w, dtype=torch.float32)) == w       # exact in fp32


# ---- 2. the exact GEMM cases ------------------------------------------------
@pytest.mark.parametrize("c", R.EXACT_CASES, ids=case_id)
def test_exact_case_is_exact(c):
    assert c.ydt in ("f32", c.xdt)                     # the ABI's rule
    assert c.n % 32 == 0 and (c.m * c.b) % 32 == 0
    g = c.g if c.g > 0 else c.n
    assert g % 32 == 0 and c.n % g == 0
    ref = R.exact_case(c)
    assert ref["abs_int"].max() < 2 ** 24
    assert np.abs(ref["y_int"]).max() < 2 ** 24
    assert np.all(np.abs(ref["y_int"]) <= ref["abs_int"])
    want32 = (ref["y_int"].astype(np.float64) / 64).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64) * 64, ref["y_int"])   # fp32 holds it
    want = ref["want"]
    assert want.dtype == R.TDT[c.ydt] and tuple(want.shape) == (c.T, c.m)
    if c.bias is not None:
        assert np.count_nonzero(ref["bias"]) > c.m // 2
    if c.ydt == "f32":
        assert np.array_equal(want.numpy(), want32)
        return
    # 16-bit output: the rounding is exercised, and so is fp16's overflow
    inexact = want.float().numpy() != want32
    assert inexact.sum() >= 10, "every exact value is representable in 16 bits"
    if c.hot and c.ydt == "f16":
        w = want.float().numpy()
        assert np.isposinf(w).any() and np.isneginf(w).any()
        assert np.isfinite(w[2:]).all() if c.T > 2 else True
    else:
        assert torch.isfinite(want.float()).all()


def test_ulp_is_the_spacing_of_the_type():
    for dt, t in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        for v in (1.0, 1.5, 3.0, 1000.0, 0.01, 6e-8 if dt == "f16" else 1e-30):
            x = torch.tensor(v, dtype=t)
            nxt = torch.nextafter(x, torch.tensor(float("inf"), dtype=t))
            assert float(nxt.double() - x.double()) == R.ulp(np.float64(float(x)), dt), (dt, v)


# ---- 3. the dispatch the shapes are meant to reach ---------------------------
@pytest.fixture(scope="module")
def L():
    import gptq_svd_amd._lib as L
    return L


def gemv_splits(L, T, m, n):
    """S of the gemv regime from the workspace query: bytes = 4 S T m + 256 with
    S the larger of the two regimes' split counts (the gemv regime's here)."""
    nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
    assert nbytes > 256 and (nbytes - 256) % (4 * T * m) == 0
    return (nbytes - 256) // (4 * T * m)


def cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("c", R.CASES_WAVE, ids=case_id)
def test_wave_shapes_reach_the_wave_loop(L, c):
    S = gemv_splits(L, c.T, c.m, c.n)
    assert 4 * S < c.n // 32, f"S = {S}: no wave owns more than one unit at {c.m} x {c.n}"
    # the last K split is short (fewer units than the others)
    ub = cdiv(c.n // 32, S)
    assert cdiv(c.n // 32, ub) == S and (c.n // 32) % ub != 0


def test_wave_shape_models(L):
    """The figures written next to the shapes in qlinear_ref.py."""
    assert gemv_splits(L, 1, R.WAVE_M, R.WAVE_N) == 13           # 5 units per workgroup
    assert gemv_splits(L, 1, R.WAVE8_M, R.WAVE8_N) == 26         # 5 units per workgroup
    # three units per wave: more than 8 units per workgroup, i.e. at most 7 splits
    # of the 64 units; 9352 is the smallest legal m (m * 4 % 32 == 0) that gets there
    assert (R.WAVE3_M * R.WAVE3_B) % 32 == 0
    assert gemv_splits(L, 1, R.WAVE3_M, R.WAVE_N) == 7
    assert cdiv(cdiv(R.WAVE_N // 32, 7), 4) == 3
    assert gemv_splits(L, 1, R.WAVE3_M - 8, R.WAVE_N) == 8       # 8 units: two per wave
    # and the shapes of the older tests do not reach the loop (why these exist)
    for m, n in ((96, 256), (64, 96), (96, 1024), (96, 512)):
        assert 4 * gemv_splits(L, 1, m, n) >= n // 32


def test_finishing_paths_of_the_output_cases(L):
    """(g): at n = 256 the mfma regime writes Y itself (no workspace above 16
    rows), at n = 1024 it goes through the partials."""
    assert L.lib.tg_qgemm_workspace_size(70, 96, 256) == 0
    assert L.lib.tg_qgemm_workspace_size(70, 96, 1024) == 2 * 70 * 96 * 4 + 256
