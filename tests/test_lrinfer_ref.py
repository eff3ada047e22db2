"""CPU: the exact data of tests/lrinfer_ref.py is exact in fp32 in any summation
order (so the bit comparisons of test_gpu_lrinfer.py cannot be vacuous), its
planted values do overflow and round in the 16-bit types, and the split
heuristic restated there is the library's, with the shapes that were chosen as
the first n at which each regime of tg_lr_down splits K."""
import ctypes

import numpy as np
import pytest
import torch

import lrinfer_ref as R


@pytest.fixture(scope="module")
def L():
    from gptq_svd_amd import _lib
    return _lib


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("T", R.TS)
def test_exact_data_is_exact(T, n):
    for r in R.RS:
        c = R.exact_case(T, n, r)
        assert c["abs_z"] < 2.0 ** 24 and c["abs_y"] < 2.0 ** 24, (T, n, r, c["abs_z"], c["abs_y"])
        for k, dts in (("X", ("f16", "bf16")), ("B", ("f16", "bf16", "f32")),
                       ("A", ("f16", "bf16", "f32")), ("bias", ("f16", "bf16", "f32"))):
            for dt in dts:
                R.as_tensor(c[k], dt)                     # asserts exactness
        R.as_tensor(c["Y32"], "f32")
        R.as_tensor(c["Z"], "f32")


def test_planted_values_overflow_and_round():
    c = R.exact_case(5, 160, 8)
    y16 = R.rounded(c["y_bias"], "f16")
    assert torch.isinf(y16).sum() >= 2 and (y16 == float("inf")).any() \
        and (y16 == float("-inf")).any()
    for dt in ("f16", "bf16"):
        y = R.rounded(c["y_bias"], dt).double().numpy()
        finite = np.isfinite(y)
        assert np.mean(y[finite] != c["y_bias"][finite]) > 0.5     # the rounding is visible
    assert np.isfinite(R.rounded(c["y_bias"], "bf16").double().numpy()).all()


def test_split_model_is_the_librarys(L):
    for T in R.TS + [2, 8, 16, 512]:
        for r in R.RS + [32]:
            for n in R.NS + [4096, 12288]:
                assert L.lib.tg_lr_down_workspace_size(T, r, n) == R.workspace_bytes(T, r, n), \
                    (T, r, n)
    assert L.lib.tg_lr_down_workspace_size(0, 8, 64) == 0


def test_smallest_splitting_shapes():
    """n = 520 is the first multiple of 8 at which the gemv regime splits K
    (chunks of at least 512 values), n = 488 the first at which the mfma regime
    does (16 slabs of 32: two splits of 8); 32 and 160 run unsplit, 1024 is
    split by both."""
    for r in R.RS:
        assert R.gemv_splits(r, 512) == 1 and R.gemv_splits(r, 520) == 2
        assert R.gemv_splits(r, 1024) == 2
        for T in R.TS:
            assert R.mfma_splits(T, r, 480) == 1 and R.mfma_splits(T, r, 488) == 2
            assert R.mfma_splits(T, r, 1024) == 4
            for n in (32, 160):
                assert R.mfma_splits(T, r, n) == 1 and R.gemv_splits(r, n) == 1
    assert R.gemv_splits(32, 4096) == 8 and R.mfma_splits(512, 32, 4096) == 16


def test_abi_rejects_bad_arguments(L):
    one = ctypes.c_void_p(256)

    def down(X=one, xdt=L.TG_F16, T=4, sx=64, B=one, bdt=L.TG_F16, r=8, n=64, sb=64, Z=one, sz=8):
        return L.lib.tg_lr_down(None, X, xdt, T, sx, B, bdt, r, n, sb, Z, sz, one, 1 << 20)

    assert down(X=None) == -2 and down(xdt=L.TG_F32) == -3 and down(T=0) == -4
    assert down(sx=63) == -5 and down(B=None) == -6 and down(bdt=L.TG_F64) == -7
    assert down(r=0) == -8 and down(r=129) == -8 and down(n=60) == -9 and down(sb=63) == -10
    assert down(Z=None) == -11 and down(sz=7) == -12
    assert L.lib.tg_lr_down(None, one, L.TG_F16, 4, 1024, one, L.TG_F16, 8, 1024, 1024, one, 8,
                            None, 0) == -13

    def fin(Y32=one, s32=104, Z=one, sz=8, A=one, adt=L.TG_F16, sa=8, T=4, m=104, r=8, bias=None,
            bdt=0, Y=one, ydt=L.TG_F16, sy=104):
        return L.lib.tg_lr_finish(None, Y32, s32, Z, sz, A, adt, sa, T, m, r, bias, bdt, Y, ydt, sy)

    assert fin(Y32=None) == -2 and fin(s32=103) == -3 and fin(Z=None) == -4 and fin(sz=7) == -5
    assert fin(A=None) == -6 and fin(adt=L.TG_F64) == -7 and fin(sa=7) == -8 and fin(T=0) == -9
    assert fin(m=0) == -10 and fin(r=129) == -11 and fin(bias=one, bdt=L.TG_F64) == -13
    assert fin(Y=None) == -14 and fin(ydt=L.TG_F64) == -15 and fin(sy=103) == -16


def test_gemv_regime_refuses_more_than_16_rows(L, monkeypatch):
    one = ctypes.c_void_p(256)
    monkeypatch.setenv("TG_LR_DOWN", "gemv")
    assert L.lib.tg_lr_down(None, one, L.TG_F16, 17, 64, one, L.TG_F16, 8, 64, 64, one, 8, one,
                            1 << 20) == -4
    assert b"gemv" in L.lib.tg_last_error()
