"""GPU: MXFP8 activations (A16) -- tg_quant_act_mx, tg_qgemm_mx_act,
quantize_act_mx / dequantize_act_mx, MXQuantLinear(act_format="mxfp8") and
load_quantized(act_format=...).  The host reference is mxa_ref.py (proved on the
CPU in test_mxa_ref.py); the weights are mx_ref.py's.  Every comparison is
bit-exact unless it says otherwise.

The random-data GEMM is held to the bound of the 16-bit kernels
(test_gpu_mx.py): |y - y64| <= TOL 2 n 2^-24 (|X^| |W^|^T) + ulp(y64) against
float64 on the quantised operands, with TOL = 1: the block-scaled MFMA met it
(worst err / bound over the cases here: see DESIGN.md "MXFP8 activations").
"""
import functools
import json

import numpy as np
import pytest
import torch

import mx_ref as W
import mxa_ref as R
from qlinear_ref import ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TDT = R.TDT
FMT, ACT = 1, 1  # TG_FMT_MXFP4, TG_ACT_MXFP8
TOL = 1.0


def lib():
    from gptq_svd_amd import _lib as L
    return L


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- 1. the quantiser -----------------------------------------------------------
def gpu_quant(x, pad):
    """x (T, n) CPU tensor -> (xq, xs) through sentinel-padded buffers: X a view
    of row stride n + pad, xq likewise, xs inside a longer byte buffer."""
    L = lib()
    T, n = x.shape
    xbuf = torch.full((T, n + pad), 7.0, dtype=x.dtype)
    xbuf[:, :n] = x
    xbuf = xbuf.to(DEV)
    qbuf = torch.full((T, n + pad), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((T * (n // 32) + 32,), 0xCD, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        L.call("tg_quant_act_mx", L.stream(), L.ptr(xbuf), L.DTYPES[x.dtype], T, n + pad, n, ACT,
               L.ptr(qbuf), n + pad, L.ptr(sbuf[16:]))
    q, s = qbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert np.all(q[:, n:] == 0xAB), "the padding of xq was written"
    assert np.all(s[:16] == 0xCD) and np.all(s[16 + T * (n // 32):] == 0xCD), \
        "bytes around xs were written"
    return q[:, :n], s[16:16 + T * (n // 32)].reshape(T, n // 32)


@pytest.mark.parametrize("pad", [5, 8])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n", [32, 160])
@pytest.mark.parametrize("T", [1, 5, 33])
def test_quantiser_bit_exact(T, n, dt, pad):
    x = R.quant_case(T, n, dt)
    want_q, want_s = R.quantize(x)
    got_q, got_s = gpu_quant(x, pad)
    assert np.array_equal(got_s, want_s), f"{np.mean(got_s != want_s):.4f} of the scale bytes differ"
    assert np.array_equal(got_q, want_q), f"{np.mean(got_q != want_q):.4f} of the bytes differ"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_quantiser_every_planted_block(dt):
    """All planted blocks at once (scale cases, ties in both directions, the
    subnormals, one large and 31 tiny values, -0, both signs of saturation),
    through the Python entry point (contiguous: the 16-byte loads and stores)."""
    from gptq_svd_amd.qlinear import dequantize_act_mx, quantize_act_mx
    pl = R.planted_blocks(dt)
    x = torch.from_numpy(np.stack([b for _, b in pl]).reshape(1, -1)).to(TDT[dt])
    x = torch.cat([x, R.quant_case(3, x.shape[1], dt)[1:]])          # (3, 32 * blocks)
    want_q, want_s = R.quantize(x)
    xq, xs = quantize_act_mx(x.to(DEV).reshape(3, 1, -1))
    assert xq.shape == (3, 1, x.shape[1]) and xs.shape == (3, 1, x.shape[1] // 32)
    assert xq.dtype == torch.uint8 and xs.dtype == torch.uint8
    assert np.array_equal(xs.cpu().numpy()[:, 0], want_s)
    assert np.array_equal(xq.cpu().numpy()[:, 0], want_q)
    assert {0x7e, 0xfe, 0x00, 0x80} <= set(want_q[0].tolist())
    back = dequantize_act_mx(xq, xs, torch.float32).cpu().numpy()[:, 0]
    normal = np.repeat(want_s >= 16, 32, axis=1)          # decoded values in fp32's normal range
    assert np.array_equal(back.view(np.uint32)[normal],
                          R.decode(want_q, want_s).view(np.uint32)[normal])


# ---- 2. / 3. the GEMM on exact integer data ---------------------------------------
def run_act(x_view, qweight, scales, m, n, y_view, bias=None):
    L = lib()
    T = x_view.shape[0]
    ldx = x_view.stride(0) if T > 1 else max(x_view.stride(0), n)
    nbytes = L.lib.tg_qgemm_mx_act_workspace_size(T, m, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm_mx_act", L.stream(), L.ptr(x_view), L.DTYPES[x_view.dtype], T, ldx,
               L.ptr(qweight), L.ptr(scales), FMT, ACT, m, n, L.ptr(bias),
               L.DTYPES[bias.dtype] if bias is not None else 0, L.ptr(y_view),
               L.DTYPES[y_view.dtype], y_view.stride(0), L.ptr(ws), nbytes)


@functools.lru_cache(maxsize=None)
def exact_case(m, n, T):
    """Weights of mx_ref.exact_gemm_case(distinct=True), activations of
    mxa_ref.exact_x; every product and partial sum an integer below 2^24."""
    c = W.exact_gemm_case(m, n, 1, 9, True)
    X = R.exact_x(T, n, T)
    y_int = X @ c["w_int"].T
    assert (np.abs(X) @ np.abs(c["w_int"]).T).max() + 100 < 2 ** 24
    qw, sc = W.pack(c["codes"], c["byte"])
    return X, y_int, qw, sc


def check_exact(m, n, T, xdt, ydt, bdt):
    """X inside a sentinel-padded buffer (stride_x > n), Y likewise (stride_y >
    m); the expected image is the exact integer result rounded once to ydt."""
    X, y_int, qw, sc = exact_case(m, n, T)
    bias = W.exact_bias(m, 3) if bdt else None
    if bias is not None:
        y_int = y_int + np.rint(bias).astype(np.int64)[None, :]
    want = torch.from_numpy(y_int.astype(F32)).to(TDT[ydt])
    pad_x = 8 if T % 2 == 0 else 5                     # 16-byte rows, or scalar loads
    SX, SY = 3.0, -12288.0
    xbuf = torch.full((T, n + pad_x), SX, dtype=TDT[xdt])
    xbuf[:, :n] = torch.from_numpy(X).to(TDT[xdt])
    xbuf = xbuf.to(DEV)
    ybuf = torch.full((T, m + 5), SY, dtype=TDT[ydt], device=DEV)
    bias_d = dev(bias, TDT[bdt]) if bdt else None
    run_act(xbuf[:, :n], dev(qw), dev(sc), m, n, ybuf[:, :m], bias=bias_d)
    got = ybuf.cpu()
    assert torch.all(got[:, m:] == SY), "the padding of Y was written"
    assert np.array_equal(W.raw_bits(got[:, :m]), W.raw_bits(want)), \
        f"{float((got[:, :m] != want).float().mean()):.4f} of the entries differ"


# 1, 15 .. 17, 33, both sides of the row tiles 16 and 64 and of the switch at T = 32, and two
# row tiles of 64 with a short second one (127 .. 129)
ROWS = (1, 15, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129)
OUT = [(ydt, bdt) for ydt in ("f16", "bf16", "f32") for bdt in (None, "f16", "bf16", "f32")]
EXACT = [(T, n, xdt) + OUT[(3 * iT + 5 * i_n + 7 * ix) % len(OUT)]
         for iT, T in enumerate(ROWS) for i_n, n in enumerate((32, 128, 160))
         for ix, xdt in enumerate(("f16", "bf16"))]
EXACT += [(17, 160, xdt) + o for xdt in ("f16", "bf16") for o in OUT]
EXACT = sorted(set(EXACT), key=EXACT.index)


@pytest.mark.parametrize("T,n,xdt,ydt,bdt", EXACT)
def test_gemm_exact(T, n, xdt, ydt, bdt):
    """m = 104: a full 64-feature tile, then two full 16-tiles and half a 16-tile
    of a partial one; n = 32 is below one MFMA K step, n = 160 a one-block tail."""
    check_exact(104, n, T, xdt, ydt, bdt)


def test_exact_cases_cover_every_output_combination():
    assert {(y, b) for _, _, _, y, b in EXACT} == set(OUT)
    assert {T for T, *_ in EXACT} == set(ROWS)


@pytest.mark.parametrize("T,xdt,ydt,bdt", [(1, "f16", "f32", None), (4, "bf16", "f32", None),
                                           (4, "f16", "f16", "f32"), (1, "bf16", "bf16", "bf16")])
def test_gemm_split_k_exact(T, xdt, ydt, bdt):
    """The smallest n at which the dispatch splits K (test_mxa_ref.py pins it):
    two splits of four K steps, finished by the reduction kernel."""
    check_exact(R.SPLIT_M, R.SPLIT_N, T, xdt, ydt, bdt)


# ---- 4. / 5. random data ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(T, n, xdt, with_bias):
    """-> x, bias, (qw, sc), y64 on the quantised operands, the bound's product term."""
    m = 104
    rng = np.random.default_rng(T + n)
    Wd = (rng.standard_normal((m, n)) * 0.05).astype(F32)
    _, codes, _, byte = W.rtn(Wd)
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(T, n, generator=gen).to(TDT[xdt])
    bias = (torch.randn(m, generator=gen) * 0.5).to(torch.float16) if with_bias else None
    xq, xs = R.quantize(x)
    x64 = R.decode(xq, xs).astype(np.float64)
    w64 = W.decode32(codes, W.expand(byte)).astype(np.float64)
    y64 = x64 @ w64.T
    if with_bias:
        y64 = y64 + bias.double().numpy()[None, :]
    return x, bias, W.pack(codes, byte), y64, np.abs(x64) @ np.abs(w64).T


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("T", [5, 40])
def test_gemm_numerics_and_determinism(T, n, xdt, with_bias):
    m = 104
    x, bias, (qw, sc), y64, prod = random_case(T, n, xdt, with_bias)
    bound = TOL * 2 * n * 2.0 ** -24 * prod + ulp(y64, xdt)
    x_d, qw_d, sc_d = x.to(DEV), dev(qw), dev(sc)
    bias_d = bias.to(DEV) if with_bias else None
    outs = []
    for _ in range(2):
        y = torch.full((T, m), float("nan"), dtype=TDT[xdt], device=DEV)
        run_act(x_d, qw_d, sc_d, m, n, y, bias=bias_d)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(W.raw_bits(outs[0]), W.raw_bits(outs[1])), "two calls differ"


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("T", [5, 40])
def test_gemm_against_the_weights_only_kernel(T, n, with_bias):
    """bf16, where X^ is exactly representable: tg_qgemm_mx_act(X) against
    tg_qgemm_mx(dequantize_act_mx(quantize_act_mx(X))) at fp32 output.  The two
    differ by summation order only: inside twice the bound of the test above."""
    from gptq_svd_amd.qlinear import dequantize_act_mx, quantize_act_mx
    from test_gpu_mx import run_qgemm_mx
    m = 104
    x, bias, (qw, sc), y64, prod = random_case(T, n, "bf16", with_bias)
    x_d, qw_d, sc_d = x.to(DEV), dev(qw), dev(sc)
    bias_d = bias.to(DEV) if with_bias else None
    xq, xs = quantize_act_mx(x_d)
    xhat = dequantize_act_mx(xq, xs, torch.bfloat16)
    assert torch.equal(xhat.float(), dequantize_act_mx(xq, xs, torch.float32))
    ya = torch.full((T, m), float("nan"), dtype=torch.float32, device=DEV)
    yw = torch.full((T, m), float("nan"), dtype=torch.float32, device=DEV)
    run_act(x_d, qw_d, sc_d, m, n, ya, bias=bias_d)
    run_qgemm_mx(xhat, qw_d, sc_d, m, n, yw, bias=bias_d)
    ulp32 = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(y64), 1e-300))) - 23)
    bound = TOL * 2 * n * 2.0 ** -24 * prod + ulp32
    diff = np.abs(ya.cpu().double().numpy() - yw.cpu().double().numpy())
    print(f"max diff / (2 bound) = {np.max(diff / (2 * bound)):.3f}")
    assert np.all(diff <= 2 * bound)
    assert np.all(np.abs(ya.cpu().double().numpy() - y64) <= bound)


# ---- 6. module and loader --------------------------------------------------------------
def test_module_forward_matches_the_abi():
    """act_format="mxfp8": leading dims flattened, a strided 3-D view, x's dtype
    returned, bias applied -- the ABI call bit for bit.  act_format=None: today's
    weights-only output bit for bit."""
    from gptq_svd_amd.qlinear import MXQuantLinear
    from test_gpu_mx import run_qgemm_mx
    m, n = 104, 160
    _, _, qw, sc = exact_case(m, n, 16)
    qw_d, sc_d = dev(qw), dev(sc)
    bias = torch.linspace(-1, 1, m).to(torch.float16).to(DEV)
    qa = MXQuantLinear.from_packed(qw_d, sc_d, bias=bias, act_format="mxfp8")
    qn = MXQuantLinear.from_packed(qw_d, sc_d, bias=bias)
    assert qa.act_format == "mxfp8" and qn.act_format is None
    assert "act_format=mxfp8" in repr(qa) and "act_format=None" in repr(qn)
    xbig = torch.randn(2, 3, n + 8, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    x = xbig[..., :n]                                        # row stride n + 8
    y = qa(x)
    assert y.shape == (2, 3, m) and y.dtype == torch.float16
    y2 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    run_act(x.reshape(6, n).contiguous(), qw_d, sc_d, m, n, y2, bias=bias)
    assert torch.equal(y.reshape(6, m), y2)
    assert torch.equal(qa(x.transpose(0, 1)), y.transpose(0, 1))
    y3 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    run_qgemm_mx(x.reshape(6, n).contiguous(), qw_d, sc_d, m, n, y3, bias=bias)
    assert torch.equal(qn(x).reshape(6, m), y3)
    assert not torch.equal(y2, y3)
    with pytest.raises(RuntimeError):
        qa(x.float())
    for bad in ("mxfp4", "int8", 8):
        with pytest.raises(ValueError):
            MXQuantLinear(n, m, act_format=bad)
        with pytest.raises(ValueError):
            MXQuantLinear.from_packed(qw_d, sc_d, act_format=bad)


def test_model_loads_with_mxfp8_activations(tmp_path):
    """The tiny random Qwen3 of test_gpu_mx.py (2 layers, 14 linears), quantised
    to MXFP4 and loaded with act_format="mxfp8": the logits against the
    weights-only ones, and against the torch emulation of the same model (each
    linear = the weights-only kernel on X^)."""
    from conftest import load_golden
    from gptq_svd_amd.export import load_quantized, save_quantized
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import MXQuantLinear, dequantize_act_mx, quantize_act_mx
    from test_gpu_mx import tiny_model
    d = load_golden("h_qwen3tiny_eigh_w4a")
    model = tiny_model(d).to(DEV)
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    res = quantize_model(model, ids, mode="eigh", eps=float(d["eps"]),
                         threshold_method=str(d["method"]), batch_size=int(d["batch"]),
                         device=DEV, pack=True, weight_format="mxfp4")
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, True, weight_format="mxfp4")
    before = sorted(p.name for p in tmp_path.iterdir())
    plain = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    act = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV,
                         act_format="mxfp8").eval()
    assert sorted(p.name for p in tmp_path.iterdir()) == before
    qmods = [mod for mod in act.modules() if isinstance(mod, MXQuantLinear)]
    assert len(qmods) == 14 and all(mod.act_format == "mxfp8" for mod in qmods)
    assert all(mod.act_format is None for mod in plain.modules()
               if isinstance(mod, MXQuantLinear))

    emul = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()

    def requantise(mod, args):
        x = args[0]
        return (dequantize_act_mx(*quantize_act_mx(x), x.dtype),)

    for mod in emul.modules():
        if isinstance(mod, MXQuantLinear):
            mod.register_forward_pre_hook(requantise)
    batch = torch.cat(ids[:4]).to(DEV)
    with torch.no_grad():
        Lw = plain(batch).logits.float()
        La = act(batch).logits.float()
        Le = emul(batch).logits.float()
    assert torch.isfinite(La).all() and not torch.equal(La, Lw)
    rel_a = float((La - Lw).norm() / Lw.norm())
    rel_e = float((Le - Lw).norm() / Lw.norm())
    print(f"|La - Lw| / |Lw| = {rel_a:.3e}, emulated {rel_e:.3e}, "
          f"|La - Le| / |Lw| = {float((La - Le).norm() / Lw.norm()):.3e}")
    assert rel_a <= 2 * rel_e, (rel_a, rel_e)

    # what is refused: an unknown format, and any format with an integer checkpoint
    with pytest.raises(ValueError):
        load_quantized(tiny_model(d).half(), str(tmp_path), act_format="mxfp6")
    qc = json.load(open(tmp_path / "quantize_config.json"))
    other = tmp_path / "int"
    other.mkdir()
    (other / "quantize_config.json").write_text(json.dumps(dict(qc, checkpoint_format="gptq_v2")))
    with pytest.raises(ValueError, match="mxfp4 checkpoint"):
        load_quantized(tiny_model(d).half(), str(other), act_format="mxfp8")
