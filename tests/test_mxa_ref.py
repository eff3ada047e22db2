"""CPU: mxa_ref.py, the numpy restatement of the MXFP8 activation contract (A16,
include/truncgptq.h), is proved here so that test_gpu_mxa.py can lean on it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mx_ref
import mxa_ref as R
from conftest import ROOT

F32 = np.float32
LIB = os.path.join(ROOT, "gptq-svd_amd", "libtruncgptq.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "gptq-svd_amd"), "-j8"], check=True)
    return ctypes.CDLL(LIB)


def all_f16():
    return torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.float16)


@pytest.mark.parametrize("k", [0, -4, 3])
def test_element_rule_is_torchs_cast(k):
    """Every fp16 bit pattern times 2^k that is finite: where |t| <= 448 the rule
    gives torch's CPU cast to float8_e4m3fn bit for bit (round to nearest even,
    subnormals kept, the sign bit kept on zeros); in (448, 512) it saturates."""
    t = all_f16().float() * 2.0 ** k
    t = t[torch.isfinite(t)]
    tn = t.numpy()
    mine = R.encode_e4m3(R.round_e4m3(tn), np.signbit(tn))
    inside = np.abs(tn) <= 448
    theirs = t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert inside.sum() > 30000
    assert np.array_equal(mine[inside], theirs[inside])
    sat = (np.abs(tn) > 448) & (np.abs(tn) < 512)
    if k == 0:
        assert sat.sum() > 100
    assert np.all(mine[sat] == np.where(tn[sat] < 0, 0xfe, 0x7e))
    # the subnormals and both zeros are among the inside values
    assert {0x00, 0x80, 0x01, 0x07, 0x08, 0x7e, 0xfe} <= set(mine[inside].tolist())


def test_decode_is_torchs_view():
    b = np.array([v for v in range(256) if v & 0x7f != 0x7f], dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).float().numpy()
    got = R.decode_e4m3(b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def expect(dt, name):
    blocks = dict(R.planted_blocks(dt))
    x = blocks[name]
    xq, xs = R.quantize(x[None, :])
    return x, xq[0], int(xs[0, 0])


def test_scale_rule_on_planted_blocks():
    # a = 4 = 2^2: field 129, byte 121, t = 64 x; the maximum lands on 256
    x, q, s = expect("f16", "pow2")
    assert s == 121 and q[5] == R.encode_e4m3(256.0, False) == 0x78
    # just below 4: field 128, byte 120, t = 128 x: 511.75 (f16) / 510 (bf16) saturate
    for dt in ("f16", "bf16"):
        x, q, s = expect(dt, "below_pow2")
        assert s == 120 and q[31] == 0xfe
    # mantissa 1.875 > 1.75: 15 -> t = 480 saturates to 448 = 14, in both signs
    x, q, s = expect("bf16", "saturate")
    assert s == 122 and list(q[[0, 1, 2, 3, 4]]) == [0x7e, 0xfe, 0x7e, 0xfe, 0x7e]
    assert np.array_equal(R.decode(q[None], np.array([[s]]))[0, :5], F32([14, -14, 14, -14, 14]))
    # a == 0: byte 0; the sign bit of -0 stays
    x, q, s = expect("f16", "zero")
    assert s == 0 and set(q.tolist()) == {0x00, 0x80} and np.array_equal(q == 0x80, np.signbit(x))
    # an fp16 subnormal maximum 3 2^-24 = 1.5 2^-23: field 104, byte 96, t = 2^31 x = 384
    x, q, s = expect("f16", "f16_subnormal")
    assert s == 96 and q[5] == R.encode_e4m3(384.0, False)
    assert np.array_equal(R.decode(q[None], np.array([[s]]))[0], x)
    # bf16 near 2^120: field 247, byte 239
    x, q, s = expect("bf16", "bf16_huge")
    assert s == 239 and q[17] == R.encode_e4m3(384.0, True)
    # a bf16 subnormal (an f32 subnormal): field 0, byte 0, t = 2^127 x = 2^-3
    x, q, s = expect("bf16", "bf16_subnormal")
    assert s == 0 and q[5] == R.encode_e4m3(0.125, False)
    assert np.array_equal(R.decode(q[None], np.array([[s]]))[0], x)


def test_rounding_on_planted_blocks():
    for dt in ("f16", "bf16"):
        x, q, s = expect(dt, "t128_ties")
        assert s == 120
        t = R.decode_e4m3(q)
        idx = [i for i in range(32) if i != 9]
        want = [16, -16, 20, -20, 224, -224, 224, -224, 18, 18, 16, -16,
                0, -0.0, 2.0 ** -8, 2.0 ** -6, -(2.0 ** -6), 2.0 ** -9, 2.0 ** -6, 2.0 ** -6,
                7 * 2.0 ** -9, 0, -0.0, 2.0 ** -6 * 1.25]
        assert np.array_equal(t[idx][:24].view(np.uint32), F32(want).view(np.uint32))
        # one large value and 31 tiny ones: the tiny ones flush to zero and keep their sign
        x, q, s = expect(dt, "large_and_tiny")
        assert s == 128 and q[30] == 0x7e                    # 1000 -> t = 500, saturated
        tiny = np.arange(32) != 30
        assert set(q[tiny].tolist()) <= {0x00, 0x80}
        assert np.array_equal(q[tiny] == 0x80, np.signbit(x[tiny]))


def test_sign_rule():
    """The sign bit of q is the sign bit of x, always."""
    for dt in ("f16", "bf16"):
        for T, n in ((5, 160), (33, 32)):
            x = R.quant_case(T, n, dt)
            xq, _ = R.quantize(x)
            assert np.array_equal((xq & 0x80) != 0, np.signbit(x.float().numpy()))
            assert not np.any((xq & 0x7f) == 0x7f)


ROWS = (1, 15, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129)


@pytest.mark.parametrize("n", [32, 128, 160, R.SPLIT_N])
def test_exact_gemm_activations_are_exact(n):
    """decode(quantize(X)) == X for the X of the exact GEMM tests, in fp16 and
    bf16, with differing scale bytes in neighbouring blocks and rows; every
    product and partial sum with the weights of mx_ref.exact_gemm_case is an
    integer below 2^24."""
    for T in ((1, 4) if n == R.SPLIT_N else ROWS):
        X = R.exact_x(T, n, T)
        for dt in ("f16", "bf16"):
            xt = torch.from_numpy(X).to(R.TDT[dt])
            assert np.array_equal(xt.double().numpy(), X.astype(np.float64))
            xq, xs = R.quantize(xt)
            assert np.array_equal(R.decode(xq, xs), X.astype(F32))
        _, xs = R.quantize(X.astype(F32))
        if n > 32:
            assert np.all(xs[:, 1:] != xs[:, :-1])
        if T > 1:
            assert np.all(xs[1:] != xs[:-1])
        m = R.SPLIT_M
        c = mx_ref.exact_gemm_case(m, n, 1, 9, True)
        assert (np.abs(X) @ np.abs(c["w_int"]).T).max() + 100 < 2 ** 24


def test_split_shape_reaches_the_split_k_path(lib):
    """The split-K shape of test_gpu_mxa.py gives more than one split and more
    than one K step per workgroup at T = 1 and 4, and one step of 128 less gives
    a single split: a later change of the dispatch constants fails here."""
    for T in (1, 4):
        S, sps = R.act_workspace_split(lib, T, R.SPLIT_M, R.SPLIT_N)
        assert S > 1 and sps > 1, (S, sps)
        assert R.act_workspace_split(lib, T, R.SPLIT_M, R.SPLIT_N - 128)[0] == 1
    # the small exact shapes run in one split
    for n in (32, 128, 160):
        assert R.act_workspace_split(lib, 33, 104, n)[0] == 1


def test_argument_errors_without_gpu(lib):
    """Both entry points reject a wrong act_fmt (and fmt) with the argument index
    before any device work."""
    lib.tg_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(256)
    i64, sz = ctypes.c_int64, ctypes.c_size_t
    rc = lib.tg_quant_act_mx(None, p, 0, 4, i64(64), 64, 2, p, i64(64), p)
    assert rc == -7 and b"argument 7" in lib.tg_last_error()
    rc = lib.tg_quant_act_mx(None, p, 0, 4, i64(64), 48, 1, p, i64(64), p)
    assert rc == -6
    rc = lib.tg_qgemm_mx_act(None, p, 0, 4, i64(64), p, p, 1, 0, 8, 64, None, 0, p, 0, i64(8), p,
                             sz(1 << 20))
    assert rc == -9 and b"argument 9" in lib.tg_last_error()
    rc = lib.tg_qgemm_mx_act(None, p, 0, 4, i64(64), p, p, 2, 1, 8, 64, None, 0, p, 0, i64(8), p,
                             sz(1 << 20))
    assert rc == -8
    rc = lib.tg_qgemm_mx_act(None, p, 0, 4, i64(64), p, p, 1, 1, 8, 64, None, 0, p, 0, i64(8), p,
                             sz(16))
    assert rc == -99


def test_module_arguments_without_gpu():
    from gptq_svd_amd.qlinear import MXQuantLinear
    assert MXQuantLinear(64, 8).act_format is None
    q = MXQuantLinear(64, 8, act_format="mxfp8")
    assert q.act_format == "mxfp8" and "act_format=mxfp8" in q.extra_repr()
    for bad in ("mxfp4", "fp8", 1):
        with pytest.raises(ValueError):
            MXQuantLinear(64, 8, act_format=bad)
