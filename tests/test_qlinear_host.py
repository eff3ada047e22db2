"""CPU: the packed-inference stage (A14) as far as it goes without a GPU --
exports and binding, the workspace query, argument errors (rejected before any
device work, so fake pointers are safe) and export.load_quantized on a CPU
model."""
import ctypes

import numpy as np
import pytest
import torch

P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced
F16, BF16, F32 = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    import gptq_svd_amd._lib as L
    return L


def test_symbols_exported_and_bound(L):
    for name in ("tg_dequant_packed", "tg_qgemm_workspace_size", "tg_qgemm"):
        assert name in L._SIGS and name in L.EXPORTED, name
    import gptq_svd_amd as pkg
    from gptq_svd_amd.qlinear import QuantLinear, dequantize_packed
    from gptq_svd_amd.export import load_quantized
    assert pkg.QuantLinear is QuantLinear and pkg.dequantize_packed is dequantize_packed
    assert pkg.load_quantized is load_quantized


def test_workspace_holds_the_split_k_partials(L):
    """truncgptq.h: S x T x m fp32 partial sums, S = 16 splits at m = n = 4096;
    the MFMA regime splits K only while its 64 x 64 output tiles are too few
    to fill the device (8 splits at T = 64, none at T = 4096)."""
    assert L.lib.tg_qgemm_workspace_size(1, 4096, 4096) >= 16 * 1 * 4096 * 4
    assert L.lib.tg_qgemm_workspace_size(16, 4096, 4096) >= 16 * 16 * 4096 * 4
    assert L.lib.tg_qgemm_workspace_size(64, 4096, 4096) >= 8 * 64 * 4096 * 4
    assert L.lib.tg_qgemm_workspace_size(4096, 4096, 4096) == 0


def qgemm(L, X=P, x_dtype=F16, T=1, ldx=None, qweight=P, qzeros=P, scales=P, scale_dtype=F16,
          m=64, n=256, group=128, w_bits=4, bias=None, bias_dtype=F16, Y=P, y_dtype=F16, ldy=None,
          ws=P, ws_bytes=1 << 30):
    return L.lib.tg_qgemm(None, X, x_dtype, T, n if ldx is None else ldx, qweight, qzeros, scales,
                          scale_dtype, m, n, group, w_bits, bias, bias_dtype, Y, y_dtype,
                          m if ldy is None else ldy, ws, ws_bytes)


def dequant(L, qweight=P, qzeros=P, scales=P, scale_dtype=F16, m=64, n=256, group=128, w_bits=4,
            out=P, out_dtype=F16, ldo=None):
    return L.lib.tg_dequant_packed(None, qweight, qzeros, scales, scale_dtype, m, n, group, w_bits,
                                   out, out_dtype, n if ldo is None else ldo)


def test_argument_errors_without_gpu(L):
    assert qgemm(L, qweight=None) == -6
    assert "argument 6" in L.last_error() and "qweight" in L.last_error()
    assert qgemm(L, w_bits=5) == -13
    assert "argument 13" in L.last_error() and "w_bits" in L.last_error()
    assert qgemm(L, n=250) == -11
    assert "argument 11" in L.last_error() and "multiple of 32" in L.last_error()
    assert qgemm(L, group=48) == -12
    assert "argument 12" in L.last_error() and "group" in L.last_error()
    assert qgemm(L, m=65, w_bits=3) == -10          # m * b is not a whole number of words
    assert qgemm(L, x_dtype=F32) == -3               # no fp32 activations
    assert qgemm(L, y_dtype=BF16) == -17             # y is x's dtype or fp32
    assert qgemm(L, ldy=63) == -18

    assert dequant(L, qweight=None) == -2
    assert "argument 2" in L.last_error() and "qweight" in L.last_error()
    assert dequant(L, w_bits=5) == -9 and "w_bits" in L.last_error()
    assert dequant(L, n=250) == -7
    assert dequant(L, group=48) == -8 and "group" in L.last_error()
    assert dequant(L, out_dtype=3) == -11


def test_forced_regime_that_cannot_take_the_shape_is_an_error(L, monkeypatch):
    monkeypatch.setenv("TG_QGEMM", "gemv")
    assert qgemm(L, T=17) == -4
    assert "argument 4" in L.last_error() and "gemv" in L.last_error()


def checkpoint(tmp_path, oracle_mod, g_idx=None):
    """The checkpoint of test_export_files_cpu: one 256 -> 64 linear with a
    bias, 4-bit asym g128, fp16 scales."""
    from gptq_svd_amd.export import save_quantized
    lin = torch.nn.Linear(256, 64, bias=True)
    model = torch.nn.Sequential()
    model.add_module("proj", lin)
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, size=(64, 256))
    scale = rng.random((64, 2)).astype(np.float32) + 0.1
    zero = rng.integers(0, 16, size=(64, 2)).astype(np.float32)
    qw, qz, sc = oracle_mod.pack_weights(codes, scale, zero, 4, False)
    packed = {"proj": dict(qweight=torch.from_numpy(qw), qzeros=torch.from_numpy(qz),
                           scales=torch.from_numpy(sc))}
    fn = save_quantized(str(tmp_path), model, packed, 4, 128, False)
    if g_idx is not None:
        from safetensors.torch import load_file, save_file
        t = load_file(fn)
        t["proj.g_idx"] = g_idx
        save_file(t, fn, metadata={"format": "pt"})
    return lin, qw, qz, sc


def fresh():
    model = torch.nn.Sequential()
    model.add_module("proj", torch.nn.Linear(256, 64, bias=True))
    return model


def test_load_quantized_cpu(tmp_path, oracle_mod):
    from gptq_svd_amd.export import load_quantized
    from gptq_svd_amd.qlinear import QuantLinear
    lin, qw, qz, sc = checkpoint(tmp_path, oracle_mod)
    model = load_quantized(fresh(), str(tmp_path))
    q = model.proj
    assert isinstance(q, QuantLinear)
    assert (q.in_features, q.out_features, q.w_bits, q.group_size) == (256, 64, 4, 128)
    assert q.qweight.dtype == torch.int32 and tuple(q.qweight.shape) == (32, 64)
    assert q.qzeros.dtype == torch.int32 and tuple(q.qzeros.shape) == (2, 8)
    assert q.scales.dtype == torch.float16 and tuple(q.scales.shape) == (2, 64)
    assert q.g_idx.dtype == torch.int32 and tuple(q.g_idx.shape) == (256,)
    assert np.array_equal(q.qweight.numpy(), qw) and np.array_equal(q.qzeros.numpy(), qz)
    assert np.array_equal(q.scales.numpy(), sc.astype(np.float16))
    assert np.array_equal(q.g_idx.numpy(), np.arange(256) // 128)
    assert torch.equal(q.bias, lin.bias.detach())
    assert set(model.state_dict()) == {"proj.qweight", "proj.qzeros", "proj.scales", "proj.g_idx",
                                       "proj.bias"}
    # the package has no CPU path and no fp32 kernel
    with pytest.raises(RuntimeError):
        model(torch.zeros(3, 256, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        q.dequantize()


def test_load_quantized_rejects_act_order(tmp_path, oracle_mod):
    import json
    import os
    from gptq_svd_amd.export import load_quantized
    perm = torch.from_numpy(np.random.default_rng(1).permutation(256) // 128).to(torch.int32)
    checkpoint(tmp_path, oracle_mod, g_idx=perm)
    with pytest.raises(ValueError, match="proj"):
        load_quantized(fresh(), str(tmp_path))
    # desc_act in the config is refused as well
    checkpoint(tmp_path, oracle_mod)
    cfg = os.path.join(str(tmp_path), "quantize_config.json")
    qc = json.load(open(cfg))
    qc["desc_act"] = True
    json.dump(qc, open(cfg, "w"))
    with pytest.raises(ValueError, match="desc_act"):
        load_quantized(fresh(), str(tmp_path))
