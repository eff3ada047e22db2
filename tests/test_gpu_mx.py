"""GPU: the MXFP4 weight format (A15) -- tg_group_params_mx, tg_gptq_quantize_mx,
tg_pack_e8m0, tg_dequant_mx, tg_qgemm_mx, MXQuantLinear and the harness /
export path.  The host reference is mx_ref.py (proved on the CPU in
test_mx_ref.py).  Every comparison is bit-exact unless it says otherwise.

The random-data GEMM uses the bound test_gpu_qlinear.py derives for the integer
kernels: |y - y64| <= 2 n 2^-24 (|X| |W^|^T) + ulp(y64), first-order fp32
accumulation in any order, doubled for the MFMA's internal grouping, plus one
output rounding.
"""
import copy
import functools
import json

import numpy as np
import pytest
import torch

import mx_ref as R
from conftest import load_golden
from qlinear_ref import ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TDT = R.TDT
FMT = 1  # TG_FMT_MXFP4


def lib():
    from gptq_svd_amd import _lib as L
    return L


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits32(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- scales -------------------------------------------------------------------
def gpu_scales(W, ldw=None):
    L = lib()
    m, n = W.shape
    ldw = n if ldw is None else ldw
    buf = torch.full((m, ldw), 1e30, dtype=torch.float32)
    buf[:, :n] = torch.from_numpy(W)
    buf = buf.to(DEV)
    scale = torch.empty((m, n // 32), dtype=torch.float32, device=DEV)
    byte = torch.empty((m, n // 32), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        L.call("tg_group_params_mx", L.stream(), L.ptr(buf), m, n, ldw, FMT, L.ptr(scale),
               L.ptr(byte))
    return scale, byte


def test_scales_planted_groups():
    """m = 5, n = 96: 15 groups; the planted maxima sit at varying lanes, in both
    signs, among smaller entries.  Row stride > n."""
    rng = np.random.default_rng(0)
    planted = [4.0, float(np.nextafter(F32(4), F32(0))), 6.0, 0.0, 1e-40, 3e38, 1.0,
               float(np.finfo(F32).tiny), float(np.finfo(F32).max), 0.75, 2.0 ** -100, 7.99]
    W = np.zeros((5, 96), dtype=F32)
    for i in range(15):
        r, g = divmod(i, 3)
        a = F32(planted[i]) if i < len(planted) else F32(np.exp(rng.uniform(-20, 20)))
        blk = (rng.uniform(-1, 1, 32) * a * 0.99).astype(F32)
        blk[(7 * i) % 32] = a if i % 2 == 0 else -a
        W[r, 32 * g:32 * g + 32] = blk
    want_scale, want_byte = R.group_scales(W)
    scale, byte = gpu_scales(W, ldw=96 + 3)
    assert np.array_equal(byte.cpu().numpy(), want_byte)
    assert np.array_equal(bits32(scale.cpu().numpy()), bits32(want_scale))
    assert want_byte.min() == 1 and want_byte.max() == 252


# ---- quantise -----------------------------------------------------------------
def gpu_quantize(W, U, perm, block, loop):
    L = lib()
    m, n = W.shape
    k = U.shape[0]
    scale, byte = gpu_scales(W)
    W_d, U_d, p_d = dev(W), dev(U.astype(F32)), dev(np.asarray(perm, dtype=np.int64))
    Wq = torch.full((m, n), float("nan"), dtype=torch.float32, device=DEV)
    codes = torch.full((m, n), 255, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        nbytes = L.lib.tg_quantize_workspace_size(m, n, block)
        ws = L.workspace(nbytes, DEV)
        L.call("tg_gptq_quantize_mx", L.stream(), L.ptr(W_d), m, n, L.ptr(U_d), k, n, L.ptr(p_d),
               L.ptr(scale), FMT, int(loop), block, L.ptr(Wq), L.ptr(codes), L.ptr(ws), nbytes)
    return Wq.cpu().numpy(), codes.cpu().numpy(), scale.cpu().numpy(), byte.cpu().numpy()


def check_quantized(got, want):
    Wq, codes, scale, byte = got
    wq, wc, ws, wb = want
    assert np.array_equal(byte, wb) and np.array_equal(bits32(scale), bits32(ws))
    assert np.array_equal(codes, wc), f"{np.mean(codes != wc):.4f} of the codes differ"
    assert np.array_equal(bits32(Wq), bits32(wq)), f"{np.mean(Wq != wq):.4f} of Wq differs"
    assert not np.any(codes == 8) and codes.max() <= 15          # -0 is never produced
    # every element is the decode of its code against its group's byte
    assert np.array_equal(bits32(Wq), bits32(R.decode32(codes, R.expand(byte))))


@pytest.mark.parametrize("loop", [0, 1])
def test_quantize_shape_one(loop):
    """m = 17 (masked rows in a second workgroup), n = 160, k = 112, block 48:
    blocks 48 / 48 / 16 (a full and a short 32-panel), two cross-block GEMMs (one
    with a short E), a 48-column RTN tail; column perm[0] holds the tie points."""
    W, U, perm, c0, planted = R.shape_one()
    want = R.gptq_fwrd_mx(W, U, perm, 48, bool(loop))
    got = gpu_quantize(W, U, perm, 48, loop)
    check_quantized(got, want)
    q, c = R.quantize_elements(planted, np.ones(17, dtype=F32))
    assert np.array_equal(got[1][:, c0], c) and np.array_equal(bits32(got[0][:, c0]), bits32(q))


@functools.lru_cache(maxsize=None)
def shape_two():
    m, n = 256, 1024
    rng = np.random.default_rng(5)
    U = np.triu(rng.standard_normal((n, n)) * (0.3 / np.sqrt(n))).astype(F32)
    U[np.arange(n), np.arange(n)] = rng.uniform(0.5, 1.5, n).astype(F32)
    perm = rng.permutation(n)
    W = (rng.standard_normal((m, n)) * np.exp(rng.uniform(-3, 3, (m, 1)))).astype(F32)
    return W, U, perm, R.gptq_fwrd_mx(W, U, perm, 1024, False)


def test_quantize_shape_two():
    """m = 256, n = k = 1024, block 1024: the look-ahead and prefetch paths of
    the block kernel at production block width."""
    W, U, perm, want = shape_two()
    check_quantized(gpu_quantize(W, U, perm, 1024, 0), want)
    assert not np.array_equal(want[1], R.rtn(W)[1])


def test_gptq_fwrd_dispatches_on_the_format():
    """Quantizer(weight_format="mxfp4") through gptq_fwrd, both use_triton
    values, and pack_quantized's MX triple."""
    from gptq_svd_amd.gptq_utils import Quantizer, gptq_fwrd, pack_quantized
    W, U, perm, _, _ = R.shape_one()
    W, U = W[:16], U                                        # m * 4 % 32 == 0 for packing
    for use_triton in (True, False):
        want = R.gptq_fwrd_mx(W, U, perm, 48, not use_triton)
        q = Quantizer(4, 32, weight_format="mxfp4")
        Wq, k = gptq_fwrd(dev(W), dev(U), q, dev(np.asarray(perm)), block_size=48,
                          use_triton=use_triton)
        assert k == 112 and np.array_equal(bits32(Wq.cpu().numpy()), bits32(want[0]))
        assert np.array_equal(q.codes.cpu().numpy(), want[1])
        assert q.scale.shape == (16, 5, 1) and q.zero.shape == (16, 5, 1)
        assert not q.zero.any() and q.scale_e8m0.dtype == torch.uint8
        assert np.array_equal(q.scale_e8m0.cpu().numpy(), want[3])
        qweight, qzeros, scales = pack_quantized(q)
        wqw, wsc = R.pack(want[1], want[3])
        assert qzeros is None and scales.dtype == torch.uint8
        assert np.array_equal(qweight.cpu().numpy(), wqw)
        assert np.array_equal(scales.cpu().numpy(), wsc)


# ---- pack and dequant -----------------------------------------------------------
BYTES = [0, 1, 103, 127, 142, 254]


@functools.lru_cache(maxsize=None)
def dequant_case():
    m, n = 264, 96                                    # > 256: one short lane block
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 16, size=(m, n)).astype(np.uint8)
    byte = rng.choice(np.array(BYTES, dtype=np.uint8), size=(m, n // 32))
    byte[:len(BYTES), 0] = BYTES
    return codes, byte


def gpu_pack(codes, byte):
    L = lib()
    m, n = codes.shape
    G = n // 32
    qweight = torch.empty((n // 8, m), dtype=torch.int32, device=DEV)
    scales = torch.empty((G, m), dtype=torch.uint8, device=DEV)
    c_d, b_d = dev(codes), dev(byte)
    with torch.cuda.device(DEV):
        L.call("tg_pack_codes", L.stream(), L.ptr(c_d), m, n, 4, L.ptr(qweight))
        L.call("tg_pack_e8m0", L.stream(), L.ptr(b_d), m, G, L.ptr(scales))
    return qweight, scales


@pytest.mark.parametrize("out", ["f16", "bf16", "f32"])
def test_pack_and_dequant(out):
    L = lib()
    codes, byte = dequant_case()
    m, n = codes.shape
    qweight, scales = gpu_pack(codes, byte)
    wqw, wsc = R.pack(codes, byte)
    assert np.array_equal(qweight.cpu().numpy(), wqw) and np.array_equal(scales.cpu().numpy(), wsc)
    ldo, SENT = n + 5, 3.0
    buf = torch.full((m, ldo), SENT, dtype=TDT[out], device=DEV)
    with torch.cuda.device(DEV):
        L.call("tg_dequant_mx", L.stream(), L.ptr(qweight), L.ptr(scales), FMT, m, n, L.ptr(buf),
               L.DTYPES[TDT[out]], ldo)
    got = buf.cpu()
    assert torch.all(got[:, n:] == SENT), "the padding of out was written"
    want = R.decode(codes, R.expand(byte), out)
    assert np.array_equal(R.raw_bits(got[:, :n]), R.raw_bits(want)), \
        f"{np.mean(R.raw_bits(got[:, :n]) != R.raw_bits(want)):.4f} of the entries differ"
    assert torch.isinf(want).any() and (want == 0).any()
    from gptq_svd_amd.qlinear import dequantize_packed_mx
    assert np.array_equal(R.raw_bits(dequantize_packed_mx(qweight, scales, TDT[out])),
                          R.raw_bits(want))


# ---- GEMM ---------------------------------------------------------------------
def run_qgemm_mx(x_view, qweight, scales, m, n, y_view, bias=None):
    L = lib()
    T = x_view.shape[0]
    ldx = x_view.stride(0) if T > 1 else max(x_view.stride(0), n)
    nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm_mx", L.stream(), L.ptr(x_view), L.DTYPES[x_view.dtype], T, ldx,
               L.ptr(qweight), L.ptr(scales), FMT, m, n, L.ptr(bias),
               L.DTYPES[bias.dtype] if bias is not None else 0, L.ptr(y_view),
               L.DTYPES[y_view.dtype], y_view.stride(0), L.ptr(ws), nbytes)


@functools.lru_cache(maxsize=None)
def exact_packed(m, n, T, seed, distinct=False):
    c = R.exact_gemm_case(m, n, T, seed, distinct)
    qw, sc = R.pack(c["codes"], c["byte"])
    return c, qw, sc


def check_exact(c, qw, sc, T, m, n, xdt, ydt, bdt, regime, monkeypatch):
    """X inside a sentinel-padded buffer (ldx > n), Y likewise (ldy > m); the
    expected image is the exact integer result rounded once to ydt."""
    monkeypatch.setenv("TG_QGEMM", regime)
    bias = R.exact_bias(m, 3) if bdt else None
    y_int = c["y_int"] + (0 if bias is None else np.rint(bias).astype(np.int64)[None, :])
    assert c["abs_int"].max() + 100 < 2 ** 24
    want = torch.from_numpy(y_int.astype(F32)).to(TDT[ydt])
    pad_x = 8 if T % 2 == 0 else 5                     # 16-byte rows, or scalar loads
    SX, SY = 3.0, -12288.0
    xbuf = torch.full((T, n + pad_x), SX, dtype=TDT[xdt])
    xbuf[:, :n] = torch.from_numpy(c["X"]).to(TDT[xdt])
    xbuf = xbuf.to(DEV)
    ybuf = torch.full((T, m + 5), SY, dtype=TDT[ydt], device=DEV)
    bias_d = dev(bias, TDT[bdt]) if bdt else None
    run_qgemm_mx(xbuf[:, :n], dev(qw), dev(sc), m, n, ybuf[:, :m], bias=bias_d)
    got = ybuf.cpu()
    assert torch.all(got[:, m:] == SY), "the padding of Y was written"
    assert np.array_equal(R.raw_bits(got[:, :m]), R.raw_bits(want)), \
        f"{float((got[:, :m] != want).float().mean()):.4f} of the entries differ"


EXACT = [(T, xdt, bdt, regime)
         for T in (1, 4, 5, 16, 33) for xdt in ("f16", "bf16") for bdt in ("f16", "bf16", "f32")
         for regime in (("gemv", "mfma", "auto") if T <= 16 else ("mfma", "auto"))]


@pytest.mark.parametrize("T,xdt,bdt,regime", EXACT)
def test_qgemm_exact(T, xdt, bdt, regime, monkeypatch):
    """m = 96 (a 64-feature tile and a partial one), n = 160 (a K tail inside a
    128-value slab); 16-bit output."""
    m, n = 96, 160
    c, qw, sc = exact_packed(m, n, T, T)
    check_exact(c, qw, sc, T, m, n, xdt, xdt, bdt, regime, monkeypatch)


@pytest.mark.parametrize("T,xdt,regime", [(5, "f16", "gemv"), (33, "bf16", "mfma")])
def test_qgemm_exact_f32_output_no_bias(T, xdt, regime, monkeypatch):
    m, n = 96, 160
    c, qw, sc = exact_packed(m, n, T, T)
    check_exact(c, qw, sc, T, m, n, xdt, "f32", None, regime, monkeypatch)


@pytest.mark.parametrize("T,xdt", [(1, "f16"), (4, "bf16")])
def test_qgemv_wave_loop(T, xdt, monkeypatch):
    """m = 4416, n = 2048: the smallest shape where a GEMV wave walks more than
    one unit (qlinear_ref.py, WAVE_M / WAVE_N) at the production dispatch;
    consecutive units carry different scale bytes, so a stale scale shows."""
    m, n = 4416, 2048
    c, qw, sc = exact_packed(m, n, 4, 9, True)
    c = dict(c, X=c["X"][:T], y_int=c["y_int"][:T], abs_int=c["abs_int"][:T])
    check_exact(c, qw, sc, T, m, n, xdt, "f32", None, "auto", monkeypatch)


NUM = [(T, n, xdt, regime, bias)
       for T in (5, 40) for n in (512,) for xdt in ("f16", "bf16")
       for regime in (("gemv", "mfma") if T <= 16 else ("mfma",)) for bias in (False,)]
NUM += [(5, 1024, "f16", "gemv", True), (40, 1024, "bf16", "mfma", True)]


@pytest.mark.parametrize("T,n,xdt,regime,with_bias", NUM)
def test_qgemm_numerics_and_determinism(T, n, xdt, regime, with_bias, monkeypatch):
    m = 96
    monkeypatch.setenv("TG_QGEMM", regime)
    rng = np.random.default_rng(T + n)
    W = (rng.standard_normal((m, n)) * 0.05).astype(F32)
    _, codes, _, byte = R.rtn(W)
    qw, sc = R.pack(codes, byte)
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(T, n, generator=gen).to(TDT[xdt])
    bias = (torch.randn(m, generator=gen) * 0.5).to(torch.float16) if with_bias else None
    w_hat = R.decode(codes, R.expand(byte), xdt)            # the operand, in x's dtype
    x64, w64 = x.double().numpy(), w_hat.double().numpy()
    y64 = x64 @ w64.T
    if with_bias:
        y64 = y64 + bias.double().numpy()[None, :]
    bound = 2 * n * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T) + ulp(y64, xdt)
    x_d, qw_d, sc_d = x.to(DEV), dev(qw), dev(sc)
    bias_d = bias.to(DEV) if with_bias else None
    outs = []
    for _ in range(2):
        y = torch.full((T, m), float("nan"), dtype=TDT[xdt], device=DEV)
        run_qgemm_mx(x_d, qw_d, sc_d, m, n, y, bias=bias_d)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(R.raw_bits(outs[0]), R.raw_bits(outs[1])), "two calls differ"


def test_mxquantlinear_forward_matches_the_abi():
    """The module: leading dims flattened, a non-contiguous input, x's dtype
    returned, bias applied, fp32 activations refused."""
    from gptq_svd_amd.qlinear import MXQuantLinear
    m, n = 96, 160
    c, qw, sc = exact_packed(m, n, 16, 16)
    qw_d, sc_d = dev(qw), dev(sc)
    bias = torch.linspace(-1, 1, m).to(torch.float16).to(DEV)
    q = MXQuantLinear.from_packed(qw_d, sc_d, bias=bias)
    xbig = torch.randn(2, 3, n + 8, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    x = xbig[..., :n]                                        # row stride n + 8
    y = q(x)
    assert y.shape == (2, 3, m) and y.dtype == torch.float16
    y2 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    run_qgemm_mx(x.reshape(6, n).contiguous(), qw_d, sc_d, m, n, y2, bias=bias)
    assert torch.equal(y.reshape(6, m), y2)
    assert torch.equal(q(x.transpose(0, 1)), y.transpose(0, 1))
    want = R.decode(c["codes"], R.expand(c["byte"]), "bf16")
    assert torch.equal(q.dequantize(torch.bfloat16).cpu(), want)
    with pytest.raises(RuntimeError):
        q(x.float())


# ---- end to end ---------------------------------------------------------------
def tiny_model(d):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    return m


def test_model_end_to_end_and_value_of_propagation(tmp_path):
    """The tiny random Qwen3 (2 layers, 14 linears): quantize_model(mxfp4,
    pack) -> save_quantized -> load_quantized; then, on layer 0's q_proj and
    k_proj, the solver's prediction error against plain MX casting of the
    original weights (test_mx_ref.py asserts the same of the host loop)."""
    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.gptq_utils import (HessianAccumulator, log_quantization_error,
                                         process_hessian_alt)
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import MXQuantLinear
    d = load_golden("h_qwen3tiny_eigh_w4a")
    model = tiny_model(d).to(DEV)
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    layer0 = model.model.layers[0]
    W0 = {n: getattr(layer0.self_attn, n).weight.detach().clone() for n in ("q_proj", "k_proj")}
    with torch.no_grad():
        x0 = layer0.input_layernorm(model.model.embed_tokens(torch.cat(ids).to(DEV)))
    res = quantize_model(model, ids, mode="eigh", eps=float(d["eps"]),
                         threshold_method=str(d["method"]), batch_size=int(d["batch"]),
                         device=DEV, pack=True, weight_format="mxfp4")
    assert all(e["weight_format"] == "mxfp4" for e in res["layer_stats"])
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, True, weight_format="mxfp4")
    tensors, qc = read_quantized(str(tmp_path))
    assert qc["checkpoint_format"] == "mxfp4" and qc["bits"] == 4 and qc["group_size"] == 32
    assert not any(k.endswith((".qzeros", ".g_idx")) for k in tensors)
    assert all(v.dtype == torch.uint8 for k, v in tensors.items() if k.endswith(".scales"))
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()

    # (a) every quantised linear was replaced and decodes to the written-back weight
    sd = model.state_dict()
    qmods = {n: mod for n, mod in packed.named_modules() if isinstance(mod, MXQuantLinear)}
    assert len(qmods) == 14 and set(qmods) == set(res["packed"])
    for n, mod in qmods.items():
        assert torch.equal(mod.dequantize(torch.float32), sd[n + ".weight"]), n

    # (b) logits: dense fp32, dense fp16 through torch's linear, packed -- the
    # closeness test_gpu_qlinear.py asks of QuantLinear
    dense16 = copy.deepcopy(model).half()
    batch = torch.cat(ids[:4]).to(DEV)
    with torch.no_grad():
        L32 = model(batch).logits.float()
        L16 = dense16(batch).logits.float()
        Lq = packed(batch).logits.float()
    e16 = float((L16 - L32).abs().max())
    eq = float((Lq - L32).abs().max())
    print(f"max|Lq - L32| = {eq:.3e}, max|L16 - L32| = {e16:.3e}, "
          f"max|Lq - L16| = {float((Lq - L16).abs().max()):.3e}")
    assert eq <= 2 * e16, (eq, e16)

    # (c) what load_quantized refuses
    cfg_file = tmp_path / "quantize_config.json"
    for change in (dict(desc_act=True), dict(checkpoint_format="mxfp8")):
        cfg_file.write_text(json.dumps(dict(qc, **change)))
        with pytest.raises(ValueError):
            load_quantized(tiny_model(d).half(), str(tmp_path))
    cfg_file.write_text(json.dumps(qc))
    bad = {n: dict(t, scales=t["scales"].to(torch.float16)) for n, t in res["packed"].items()}
    with pytest.raises(ValueError, match="uint8"):
        save_quantized(str(tmp_path / "bad"), model, bad, 4, 32, True, weight_format="mxfp4")
    from safetensors.torch import save_file
    wrong = {k: (v.to(torch.float16) if k.endswith(".scales") else v) for k, v in tensors.items()}
    save_file(wrong, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    with pytest.raises(ValueError, match="uint8"):
        load_quantized(tiny_model(d).half(), str(tmp_path))

    # (d) the value of the propagation
    acc = HessianAccumulator(x0.shape[-1], DEV)
    acc.add_batch(x0)
    _, R_x, perm = process_hessian_alt(acc.get_hessian(), float(d["eps"]), str(d["method"]))
    for n, W in W0.items():
        Wq = sd[f"model.layers.0.self_attn.{n}.weight"]
        e_solver = log_quantization_error(W, Wq, R_x, perm)
        e_rtn = log_quantization_error(W, dev(R.rtn(W.cpu().numpy())[0]), R_x, perm)
        print(f"{n}: solver {e_solver:.4f}, plain casting {e_rtn:.4f}")
        assert e_solver < e_rtn


def test_run_and_record_evaluates_the_mx_checkpoint(tmp_path):
    """evaluate_packed with the new format: the checkpoint is written as mxfp4,
    loaded into MXQuantLinear modules, and the run config records the format."""
    import os
    from gptq_svd_amd.harness import run_and_record
    from gptq_svd_amd.qlinear import MXQuantLinear
    d = load_golden("h_qwen3tiny_eigh_w4a")
    model = tiny_model(d).to(DEV)
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    seen = {}

    def fake_ppl(m):
        seen["mx"] = sum(isinstance(x, MXQuantLinear) for x in m.modules())
        with torch.no_grad():
            return float(m(torch.cat(ids[:2]).to(DEV)).logits.float().abs().mean())

    run_and_record(model, ids, str(tmp_path), evaluate_packed=fake_ppl, mode="eigh",
                   eps=float(d["eps"]), threshold_method=str(d["method"]),
                   batch_size=int(d["batch"]), device=DEV, weight_format="mxfp4")
    assert seen["mx"] == 14
    out = json.load(open(os.path.join(str(tmp_path), "results.json")))
    assert out["config"]["weight_format"] == "mxfp4" and out["config"]["w_bits"] == 4
    assert out["config"]["group_size"] == 32 and np.isfinite(out["metrics"]["packed_ppl"])
    qc = json.load(open(os.path.join(str(tmp_path), "packed", "quantize_config.json")))
    assert qc["checkpoint_format"] == "mxfp4"
