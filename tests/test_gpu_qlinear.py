"""GPU: packed inference (A14) -- tg_dequant_packed, tg_qgemm (both regimes),
QuantLinear and export.load_quantized.

Host references come from the oracle's packer / unpacker and numpy / torch on
the CPU; the helpers (packed_case, host_dequant, exact_reference, raw_bits,
ulp, regimes) live in qlinear_ref.py, shared with test_gpu_qlinear_edges.py
(production dispatch and layout edges) and checked on the CPU in
test_qlinear_ref.py:

1. dequant: bit-exact against float32(code - zero) * float32(scale) rounded
   once to the output type.
2. GEMM layout: integer X in [-2, 2], power-of-two scales, fp32 output: every
   product and partial sum is an exact fp32 multiple of 2^-6 below 2^24, so the
   result must equal the host int64 computation exactly, in any summation
   order.  Strided X and Y, Y's padding untouched, asymmetric data.
3. GEMM numerics on random data: |y - y64| <= 2 n 2^-24 (|X| |W^|^T) + ulp(y64)
   (first-order bound of fp32 accumulation in any order, doubled for the MFMA's
   internal grouping, plus one output rounding; derived, not measured), and the
   same call twice gives the same bits.
4. End to end on the tiny Qwen3 goldens: quantise, save, load_quantized; the
   decoded weights are the written-back ones bit for bit; the packed model's
   logits are as close to the fp32 model's as twice what torch's own fp16
   linear manages; evaluate_perplexity runs on the packed model.
   Measured on an MI355X (also in DESIGN.md), 4 x 32 calibration tokens:
     h_qwen3tiny_eigh_w3s_mt: max|Lq - L32| = 1.036e-3, max|L16 - L32| = 1.036e-3,
                              PPL packed 258.8253, dense fp16 258.8253
     h_qwen3tiny_gptq_w4a:    max|Lq - L32| = 1.178e-3, max|L16 - L32| = 1.178e-3,
                              PPL packed 260.3776, dense fp16 260.3776
   (Lq and L16 agree in every logit at these sizes: K = 128 / 256 fits one or
   two K slabs and the MFMA adds them in the same order as torch's GEMM.)
"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from qlinear_ref import (BITS, TDT, exact_reference, host_dequant, packed_case, raw_bits,
                         regimes, ulp)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from eval_corpus import ByteTokenizer, corpus  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

def to_dev(qw, qz, sc, scale_dtype):
    return (torch.from_numpy(qw).to(DEV), torch.from_numpy(qz).to(DEV),
            torch.from_numpy(sc).to(scale_dtype).to(DEV))


# ---- 1. dequant ---------------------------------------------------------------
@pytest.mark.parametrize("out", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("sdt", ["f16", "f32"])
@pytest.mark.parametrize("b", BITS)
@pytest.mark.parametrize("shape", [(64, 256, 128), (96, 96, 32), (32, 128, -1)])
def test_dequant_bit_exact(shape, b, sdt, out):
    from gptq_svd_amd.qlinear import dequantize_packed
    m, n, g = shape
    codes, zero, scale, qw, qz, sc = packed_case(m, n, g, b, "rand")
    qw_d, qz_d, sc_d = to_dev(qw, qz, sc, TDT[sdt])
    got = dequantize_packed(qw_d, qz_d, sc_d, b, g, TDT[out])
    assert got.shape == (m, n) and got.dtype == TDT[out]
    scale_used = sc_d.cpu().float().numpy().T          # (m, G), after the fp16 rounding if any
    want = host_dequant(codes, zero, scale_used, g, out)
    assert np.array_equal(raw_bits(got), raw_bits(want)), \
        f"{np.mean(raw_bits(got) != raw_bits(want)):.3f} of the entries differ"


# ---- 2 / 3. GEMM ------------------------------------------------------------
def run_qgemm(x_view, qw_d, qz_d, sc_d, m, n, g, b, y_view, bias=None):
    """The C ABI directly (QuantLinear.forward allocates its own dense Y)."""
    from gptq_svd_amd import _lib as L
    T = x_view.shape[0]
    ldx = x_view.stride(0) if T > 1 else max(x_view.stride(0), n)
    nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm", L.stream(), L.ptr(x_view), L.DTYPES[x_view.dtype], T, ldx,
               L.ptr(qw_d), L.ptr(qz_d), L.ptr(sc_d), L.DTYPES[sc_d.dtype], m, n, g, b,
               L.ptr(bias), L.DTYPES[bias.dtype] if bias is not None else 0, L.ptr(y_view),
               L.DTYPES[y_view.dtype], y_view.stride(0), L.ptr(ws), nbytes)


EXACT = [(T, shape, b, xdt, regime)
         for T in (1, 3, 16, 17, 33, 130)
         for shape in ((96, 256, 128), (64, 96, 32))
         for b in BITS for xdt in ("f16", "bf16") for regime in regimes(T)]
# n = 1024: the mfma regime splits K too (two splits of four 128-value slabs);
# T = 70 and 200 take its 128-row tile (one short tile; two tiles, the last short)
EXACT += [(T, (96, 1024, 128), b, xdt, regime)
          for T in (3, 70) for b in (3, 4) for xdt in ("f16", "bf16") for regime in regimes(T)]
EXACT += [(200, (96, 256, 128), b, xdt, "mfma") for b in (3, 4) for xdt in ("f16", "bf16")]


@pytest.mark.parametrize("T,shape,b,xdt,regime", EXACT)
def test_qgemm_layout_exact(T, shape, b, xdt, regime, monkeypatch):
    m, n, g = shape
    monkeypatch.setenv("TG_QGEMM", regime)
    codes, zero, scale, qw, qz, sc = packed_case(m, n, g, b, "pow2")
    qw_d, qz_d, sc_d = to_dev(qw, qz, sc, torch.float16)
    rng = np.random.default_rng(T * 31 + b)
    X = rng.integers(-2, 3, size=(T, n))
    # ldx > n: a multiple of 8 (16-byte rows) for even T, odd otherwise
    pad_x = 8 if T % 2 == 0 else 5
    xbuf = torch.full((T, n + pad_x), 3.0, dtype=TDT[xdt])
    xbuf[:, :n] = torch.from_numpy(X).to(TDT[xdt])
    xbuf = xbuf.to(DEV)
    SENT = 777.0
    ybuf = torch.full((T, m + 5), SENT, dtype=torch.float32, device=DEV)
    run_qgemm(xbuf[:, :n], qw_d, qz_d, sc_d, m, n, g, b, ybuf[:, :m])
    # host: integers scaled by 2^6 (scales are 2^-6 .. 2^-2)
    want, y_int, _ = exact_reference(X, codes, zero, scale, g)
    assert np.abs(y_int).max() < 2 ** 24
    want = want.numpy()
    got = ybuf.cpu().numpy()
    assert np.all(got[:, m:] == SENT), "padding of Y was written"
    assert np.array_equal(got[:, :m], want), \
        f"{np.mean(got[:, :m] != want):.3f} of the entries differ"


NUM = [(T, 512, b, xdt, regime, bias)
       for T in (5, 40) for b in (3, 4) for xdt in ("f16", "bf16") for regime in regimes(T)
       for bias in (False,)] + [(5, 512, 4, "f16", "gemv", True), (5, 512, 4, "f16", "mfma", True),
                                (40, 512, 4, "f16", "mfma", True),
                                # n = 1024: split K in the mfma regime as well
                                (40, 1024, 4, "f16", "mfma", True),
                                (40, 1024, 3, "bf16", "mfma", False),
                                (5, 1024, 4, "f16", "gemv", True)]


@pytest.mark.parametrize("T,n,b,xdt,regime,with_bias", NUM)
def test_qgemm_numerics_and_determinism(T, n, b, xdt, regime, with_bias, monkeypatch):
    m, g = 96, 128
    monkeypatch.setenv("TG_QGEMM", regime)
    codes, zero, scale, qw, qz, sc = packed_case(m, n, g, b, "small")
    qw_d, qz_d, sc_d = to_dev(qw, qz, sc, torch.float32)
    gen = torch.Generator().manual_seed(T + b)
    x = torch.randn(T, n, generator=gen).to(TDT[xdt])
    bias = (torch.randn(m, generator=gen) * 0.5).to(torch.float16) if with_bias else None
    w_hat = host_dequant(codes, zero, scale, g, xdt)        # the operand, in x's dtype
    x64, w64 = x.double().numpy(), w_hat.double().numpy()
    y64 = x64 @ w64.T
    if with_bias:
        y64 = y64 + bias.double().numpy()[None, :]
    bound = 2 * n * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T) + ulp(y64, xdt)
    x_d = x.to(DEV)
    bias_d = bias.to(DEV) if with_bias else None
    outs = []
    for _ in range(2):
        y = torch.full((T, m), float("nan"), dtype=TDT[xdt], device=DEV)
        run_qgemm(x_d, qw_d, qz_d, sc_d, m, n, g, b, y, bias=bias_d)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(raw_bits(outs[0]), raw_bits(outs[1])), "two calls differ"


def test_quantlinear_forward_matches_the_abi():
    """The module: leading dims flattened, x's dtype returned, bias applied,
    fp32 activations refused."""
    from gptq_svd_amd.qlinear import QuantLinear
    m, n, g, b = 96, 512, 128, 4
    codes, zero, scale, qw, qz, sc = packed_case(m, n, g, b, "small")
    qw_d, qz_d, sc_d = to_dev(qw, qz, sc, torch.float16)
    bias = torch.linspace(-1, 1, m).to(torch.float16).to(DEV)
    q = QuantLinear.from_packed(qw_d, qz_d, sc_d, b, g, bias=bias)
    x = torch.randn(2, 3, n, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    y = q(x)
    assert y.shape == (2, 3, m) and y.dtype == torch.float16
    y2 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    run_qgemm(x.reshape(6, n), qw_d, qz_d, sc_d, m, n, g, b, y2, bias=bias)
    assert torch.equal(y.reshape(6, m), y2)
    want = host_dequant(codes, zero, sc_d.cpu().float().numpy().T, g, "f16")
    assert torch.equal(q.dequantize(torch.float16).cpu(), want)
    with pytest.raises(RuntimeError):
        q(x.float())


# ---- 4. end to end ------------------------------------------------------------
def tiny_model(d, weights="init"):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    return m


@pytest.mark.parametrize("name", golden_names("h_")[:1] + golden_names("h_")[-1:])
def test_packed_model_end_to_end(name, tmp_path):
    from gptq_svd_amd import evaluate as ev
    from gptq_svd_amd.export import load_quantized, save_quantized
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import QuantLinear
    d = load_golden(name)
    bits, group, sym = int(d["bits"]), int(d["group"]), bool(d["sym"])
    model = tiny_model(d).to(DEV)
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    res = quantize_model(model, ids, mode=str(d["mode"]), w_bits=bits, group_size=group, sym=sym,
                         eps=float(d["eps"]), threshold_method=str(d["method"]),
                         actorder=bool(d["actorder"]), batch_size=int(d["batch"]), device=DEV,
                         pack=True)
    save_quantized(str(tmp_path), model, res["packed"], bits, group, sym,
                   scale_dtype=torch.float32)
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()

    # (a) every quantised linear was replaced and decodes to the written-back weight
    sd = model.state_dict()
    qmods = {n: mod for n, mod in packed.named_modules() if isinstance(mod, QuantLinear)}
    assert len(qmods) == 14 and set(qmods) == set(res["packed"])
    for n, mod in qmods.items():
        assert mod.scales.dtype == torch.float32
        assert torch.equal(mod.dequantize(torch.float32), sd[n + ".weight"]), n

    # (b) logits: dense fp32, dense fp16 through torch's linear, packed
    dense16 = copy.deepcopy(model).half()
    batch = torch.cat(ids[:4]).to(DEV)
    with torch.no_grad():
        L32 = model(batch).logits.float()
        L16 = dense16(batch).logits.float()
        Lq = packed(batch).logits.float()
    e16 = float((L16 - L32).abs().max())
    eq = float((Lq - L32).abs().max())
    print(f"{name}: max|Lq - L32| = {eq:.3e}, max|L16 - L32| = {e16:.3e}, "
          f"max|Lq - L16| = {float((Lq - L16).abs().max()):.3e}, "
          f"{float((Lq != L16).float().mean()):.3f} of the logits differ")
    assert eq <= 2 * e16, (eq, e16)

    # (c) the evaluator runs on the packed model (values recorded, not gated)
    lines = corpus(11, 40)
    kw = dict(device=DEV, batch_size=4, stride=32, text=lines)
    ppl_q = ev.evaluate_perplexity(packed, ByteTokenizer(), "wikitext2", **kw)
    ppl_16 = ev.evaluate_perplexity(dense16, ByteTokenizer(), "wikitext2", **kw)
    print(f"{name}: PPL packed {ppl_q:.4f}, dense fp16 {ppl_16:.4f}")
    assert np.isfinite(ppl_q)


def test_run_and_record_evaluates_the_packed_checkpoint(tmp_path):
    """evaluate_packed (opt-in): the checkpoint is written, loaded back into
    QuantLinear modules and its perplexity lands in metrics.packed_ppl."""
    from gptq_svd_amd import evaluate as ev
    from gptq_svd_amd.harness import run_and_record
    from gptq_svd_amd.qlinear import QuantLinear
    d = load_golden(golden_names("h_")[-1])
    model = tiny_model(d).to(DEV)
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    seen = {}

    def ppl_of_packed(m):
        seen["quant"] = sum(isinstance(x, QuantLinear) for x in m.modules())
        seen["ppl"] = ev.evaluate_perplexity(m, ByteTokenizer(), "wikitext2", device=DEV,
                                             batch_size=4, stride=32, text=corpus(11, 20))
        return seen["ppl"]

    run_and_record(model, ids, str(tmp_path), evaluate_packed=ppl_of_packed, mode=str(d["mode"]),
                   w_bits=int(d["bits"]), group_size=int(d["group"]), sym=bool(d["sym"]),
                   eps=float(d["eps"]), threshold_method=str(d["method"]),
                   actorder=bool(d["actorder"]), batch_size=int(d["batch"]), device=DEV)
    assert seen["quant"] == 14
    assert not any(isinstance(x, QuantLinear) for x in model.modules())  # the dense model stays
    metrics = json.load(open(os.path.join(str(tmp_path), "results.json")))["metrics"]
    assert metrics["packed_ppl"] == seen["ppl"] and np.isfinite(metrics["packed_ppl"])
    assert "quantized_ppl" not in metrics
    assert os.path.exists(os.path.join(str(tmp_path), "packed", "model.safetensors"))
