"""Act-order checkpoints (A21) through QuantLinear, dequantize_packed and
load_quantized.  The layer: the oracle's packing of random codes / zeros /
scales in checkpoint order and g_idx[perm[j]] = j // g for a random perm; m = 96
(one and a half feature tiles), n = 512 (several K splits, 8 or 4 groups).

1. repack / dequant exact; 2. forward bit for bit the static module on the
sorted stream fed x[:, col_perm] (sorted position order is the summation order
of both), each of tg_qgemm's regimes forced in turn: gemv takes the fused
gather, mfma the gather launch; 3. forward against float64 with the bar of
test_gpu_qlinear.py (operand = W_ref rounded once to x's dtype, |y - y64| <=
2 n 2^-24 |x| |W^|^T + ulp(y64)); 4. rotation / low-rank; 5. the loader;
6. refusals and argument errors (no device call is reached; unmarked).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from qlinear_ref import BITS, TDT, oracle, packed_case, raw_bits, regimes, ulp

gpu = pytest.mark.gpu
DEV = "cuda:0"
M, N = 96, 512


def permuted_g_idx(n, g, seed):
    perm = np.random.default_rng(seed).permutation(n)
    g_idx = np.empty(n, dtype=np.int32)
    g_idx[perm] = np.arange(n) // g
    return g_idx


@functools.lru_cache(maxsize=None)
def layer(b, g):
    """Host side of one act-order layer; callers leave the arrays unchanged."""
    codes, zero, scale, qw, qz, sc = packed_case(M, N, g, b, "small")
    g_idx = permuted_g_idx(N, g, 10 * b + g)
    col_perm = np.argsort(g_idx, kind="stable")
    w32 = (codes - zero[:, g_idx]).astype(np.float32) * scale[:, g_idx]
    assert w32.dtype == np.float32
    qw_sorted = oracle().pack_weights(codes[:, col_perm], scale, zero.astype(np.float32), b,
                                      False)[0]
    return dict(qw=qw, qz=qz, sc=sc, g_idx=g_idx, col_perm=col_perm, w32=w32, qw_sorted=qw_sorted)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def modules(b, g, with_bias=False):
    """(act-order module, static module of the sorted stream), fp32 scales."""
    from gptq_svd_amd.qlinear import QuantLinear
    L = layer(b, g)
    bias = torch.linspace(-1, 1, M).to(torch.float16).to(DEV) if with_bias else None
    qz, sc = dev(L["qz"]), dev(L["sc"])
    act = QuantLinear.from_packed(dev(L["qw"]), qz, sc, b, g, bias=bias, g_idx=dev(L["g_idx"]),
                                  act_order=True)
    static = QuantLinear.from_packed(dev(L["qw_sorted"]), qz, sc, b, g, bias=bias)
    return act, static


def random_x(T, xdt, pad=0):
    """(T, N) view with row stride N + pad of random activations on the device."""
    x = torch.randn(T, N + pad, generator=torch.Generator().manual_seed(T)).to(TDT[xdt]).to(DEV)
    return x[:, :N]


# ---- 1. repack and dequant ------------------------------------------------------
@gpu
@pytest.mark.parametrize("g", [64, 128])
@pytest.mark.parametrize("b", BITS)
def test_repack_and_dequant_exact(b, g):
    from gptq_svd_amd.qlinear import dequantize_packed
    L = layer(b, g)
    got = dequantize_packed(dev(L["qw"]), dev(L["qz"]), dev(L["sc"]), b, g, dtype=torch.float32,
                            g_idx=dev(L["g_idx"]))
    assert np.array_equal(raw_bits(got), raw_bits(torch.from_numpy(L["w32"])))
    act, _ = modules(b, g)
    assert np.array_equal(act.col_perm.cpu().numpy(), L["col_perm"])
    assert act.col_perm.dtype == torch.int32 and "col_perm" not in act.state_dict()
    assert np.array_equal(act.g_idx.cpu().numpy(), L["g_idx"])
    assert np.array_equal(act.qweight.cpu().numpy(), L["qw_sorted"]), "sorted stream"
    want16 = torch.from_numpy(L["w32"]).to(torch.float16)
    assert np.array_equal(raw_bits(act.dequantize()), raw_bits(want16))


# ---- 2. forward against the static kernel ---------------------------------------
@gpu
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("T,regime", [(T, r) for T in (1, 5, 16, 17, 80) for r in regimes(T)])
@pytest.mark.parametrize("g", [64, 128])
@pytest.mark.parametrize("b", BITS)
def test_forward_is_the_static_kernel_on_gathered_x(b, g, T, regime, xdt, monkeypatch):
    monkeypatch.setenv("TG_QGEMM", regime)
    act, static = modules(b, g)
    x = random_x(T, xdt, pad=5 if T in (5, 17) else 0)      # ldx > n, rows not 16-byte aligned
    cp = act.col_perm.long()
    got, want = act(x), static(x[:, cp])
    assert got.shape == (T, M) and got.dtype == TDT[xdt]
    assert torch.equal(got, want), f"{float((got != want).float().mean()):.3f} of the entries differ"


@gpu
@pytest.mark.parametrize("T", [1, 16, 17])
def test_forward_default_dispatch_and_vector_stride(T):
    """TG_QGEMM unset, x with ldx = n + 8 (16-byte rows: the gather's vector loads)."""
    act, static = modules(4, 128, True)
    x = random_x(T, "f16", pad=8)
    assert torch.equal(act(x), static(x[:, act.col_perm.long()]))


@gpu
@pytest.mark.parametrize("n,T,pad", [(4096, 6, 0), (4128, 6, 8), (8224, 1, 5)])
def test_gather_cols_row_segments(n, T, pad):
    """Rows longer than one LDS segment of 4096 columns (the last segment short),
    a short last block of rows, vector and scalar loads."""
    from gptq_svd_amd import _lib as L
    gen = torch.Generator().manual_seed(n + T)
    x = torch.randn(T, n + pad, generator=gen).half().to(DEV)[:, :n]
    cp = torch.randperm(n, generator=gen).to(torch.int32).to(DEV)
    y = torch.zeros(T, n, dtype=torch.float16, device=DEV)
    with torch.cuda.device(DEV):
        L.call("tg_gather_cols", L.stream(), L.ptr(x), L.TG_F16, T, n + pad, n, L.ptr(cp), L.ptr(y),
               n)
    assert torch.equal(y, x[:, cp.long()])


# ---- 3. forward against float64 -------------------------------------------------
@gpu
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("g", [64, 128])
@pytest.mark.parametrize("b", BITS)
def test_forward_numerics(b, g, T, xdt):
    act, _ = modules(b, g, True)
    x = random_x(T, xdt)
    check_against_float64(act(x), x, layer(b, g)["w32"], act.bias, xdt)


def check_against_float64(y, x, w32, bias, xdt):
    w64 = torch.from_numpy(w32).to(TDT[xdt]).double().numpy()     # the operand, in x's dtype
    x64 = x.cpu().double().numpy()
    y64 = x64 @ w64.T + bias.cpu().double().numpy()[None, :]
    bound = 2 * x64.shape[1] * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T) + ulp(y64, xdt)
    err = np.abs(y.cpu().double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"


# ---- 4. composition -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("T", [3, 40])
def test_rotation_composes(T):
    """The rotated x is what is gathered."""
    from gptq_svd_amd.qlinear import QuantLinear, hadamard
    b, g, block = 4, 128, 128
    L = layer(b, g)
    sign = torch.randint(-2 ** 31, 2 ** 31 - 1, (N // 32,), dtype=torch.int64,
                         generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    act = QuantLinear.from_packed(dev(L["qw"]), dev(L["qz"]), dev(L["sc"]), b, g,
                                  g_idx=dev(L["g_idx"]), rotation=(block, sign), act_order=True)
    _, static = modules(b, g)
    x = random_x(T, "f16")
    want = static(hadamard(x, block, sign)[:, act.col_perm.long()])
    assert torch.equal(act(x), want)


@gpu
@pytest.mark.parametrize("T", [3, 40])
def test_lowrank_composes(T):
    """The correction is computed from the ungathered x: the static GEMM's fp32
    sums on the gathered x, finished by the same tg_lr_down / tg_lr_finish."""
    from gptq_svd_amd import qlinear as Q
    b, g, r = 4, 128, 8
    L = layer(b, g)
    gen = torch.Generator().manual_seed(2)
    A = (torch.randn(M, r, generator=gen) * 0.1).half().to(DEV)
    B = (torch.randn(r, N, generator=gen) * 0.1).half().to(DEV)
    bias = torch.linspace(-1, 1, M).half().to(DEV)
    act = Q.QuantLinear.from_packed(dev(L["qw"]), dev(L["qz"]), dev(L["sc"]), b, g, bias=bias,
                                    g_idx=dev(L["g_idx"]), lowrank=(A, B), act_order=True)
    _, static = modules(b, g)
    x = random_x(T, "f16")
    xg = x[:, act.col_perm.long()].contiguous()
    y32 = torch.empty(T, M, dtype=torch.float32, device=DEV)
    want = torch.empty(T, M, dtype=torch.float16, device=DEV)
    with torch.cuda.device(DEV):
        static._gemm(xg, T, N, None, y32)
        Q._lowrank_finish(x, T, N, y32, A, B, bias, want)
    assert torch.equal(act(x), want)


# ---- 5. loader ------------------------------------------------------------------
@gpu
def test_load_quantized_act_order(tmp_path, oracle_mod):
    from gptq_svd_amd.export import load_quantized
    from test_qlinear_host import checkpoint, fresh
    n, m, g, b = 256, 64, 128, 4
    g_idx = permuted_g_idx(n, g, 3)
    lin, qw, qz, sc = checkpoint(tmp_path, oracle_mod, g_idx=torch.from_numpy(g_idx))
    cfg = os.path.join(str(tmp_path), "quantize_config.json")
    qc = json.load(open(cfg))
    qc["desc_act"] = True
    json.dump(qc, open(cfg, "w"))
    q = load_quantized(fresh(), str(tmp_path), device=DEV, act_order=True).proj
    assert q.col_perm is not None and q.col_perm.device.type == "cuda"
    codes = oracle_mod.unpack_rows_bitstream(qw, b, n).T
    zero = oracle_mod.unpack_rows_bitstream(qz.T.copy(), b, m)
    scale = sc.astype(np.float16).astype(np.float32).T            # fp16 in the checkpoint
    w32 = (codes - zero[:, g_idx]).astype(np.float32) * scale[:, g_idx]
    x = torch.randn(17, n, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    check_against_float64(q(x), x, w32, q.bias, "f16")

    # a trivial g_idx under act_order=True is the static module
    checkpoint(tmp_path, oracle_mod)
    q1 = load_quantized(fresh(), str(tmp_path), device=DEV, act_order=True).proj
    q0 = load_quantized(fresh(), str(tmp_path), device=DEV).proj
    assert q1.col_perm is None
    assert torch.equal(q1(x), q0(x))


# ---- 6. refusals ----------------------------------------------------------------
def cpu_layer(g_idx, **kw):
    from gptq_svd_amd.qlinear import QuantLinear
    L = layer(4, 128)
    return QuantLinear.from_packed(torch.from_numpy(L["qw"]), torch.from_numpy(L["qz"]),
                                   torch.from_numpy(L["sc"]), 4, 128,
                                   g_idx=torch.from_numpy(g_idx), act_order=True, **kw)


@pytest.mark.parametrize("case", ["out_of_range", "short_group", "int8"])
def test_refusals(case):
    g_idx = layer(4, 128)["g_idx"].copy()
    kw = {}
    if case == "out_of_range":
        g_idx[7] = N // 128
    elif case == "short_group":                 # one group of g - 1 columns, one of g + 1
        g_idx[np.flatnonzero(g_idx == 0)[0]] = 1
    else:
        kw["act_format"] = "int8"
    with pytest.raises(ValueError):
        cpu_layer(g_idx, **kw)


def test_argument_errors_without_gpu():
    """Rejected with the argument's index before any device work."""
    import ctypes
    from gptq_svd_amd import _lib as L
    P, P2 = ctypes.c_void_p(4096), ctypes.c_void_p(8192)      # non-null, never dereferenced
    base = {"tg_qgemm_gidx": [None, P, 0, 1, 256, P, P, P, 0, 64, 256, 128, 4, None, 0, P2, 0, 64,
                              P, 1 << 30, P],
            "tg_dequant_gidx": [None, P, P, P, 0, 64, 256, 128, 4, P2, 0, 256, P],
            "tg_repack_gidx": [None, P, P, 64, 256, 4, P2],
            "tg_gather_cols": [None, P, 0, 1, 256, 256, P, P2, 256]}
    for name, idx, bad in (("tg_qgemm_gidx", 21, None), ("tg_qgemm_gidx", 5, 255),
                           ("tg_qgemm_gidx", 12, 48), ("tg_dequant_gidx", 13, None),
                           ("tg_dequant_gidx", 7, 250), ("tg_dequant_gidx", 12, 255),
                           ("tg_repack_gidx", 7, P), ("tg_repack_gidx", 5, 250),
                           ("tg_gather_cols", 9, 255), ("tg_gather_cols", 3, 2)):
        args = list(base[name])
        args[idx - 1] = bad
        rc = getattr(L.lib, name)(*args)
        assert rc == -idx and f"argument {idx}:" in L.last_error(), (name, idx, rc, L.last_error())
