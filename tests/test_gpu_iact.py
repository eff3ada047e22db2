"""GPU: INT8 activations for integer checkpoints (A20) -- tg_quant_act_i8,
tg_qgemm_act, QuantLinear(act_format="int8") and load_quantized(act_format="int8")
against iact_ref.py.  Every comparison is bit-exact but the random-data GEMM,
which is held to the forward-error bound of the contract's own operation count,
(G + 4) 2^-24 (xs sum_j |D| scale + |bias|) + ulp(y64); the worst err / bound
measured over the cases here is in DESIGN.md "INT8 activations (A20)"."""
import json

import numpy as np
import pytest
import torch

import iact_ref as R
from qlinear_ref import TDT, raw_bits, ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT = 2  # TG_ACT_INT8


def lib():
    from gptq_svd_amd import _lib as L
    return L


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- 1. the quantiser ---------------------------------------------------------------
@pytest.mark.parametrize("pad", [5, 8])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n", [32, 160])
@pytest.mark.parametrize("T", [1, 5, 33])
def test_quantiser_bit_exact(T, n, dt, pad):
    """Random rows, then the planted ones: all zero, +-max alone (+-127, never
    -128), rounding ties at xs = 1 in both directions, and -0.  X and xq are views
    of row stride n + pad inside sentinel buffers, xs and xsum inside longer ones."""
    L = lib()
    x = torch.randn(T + 3, n, generator=torch.Generator().manual_seed(T + n)) * 3
    x[T] = 0
    x[T + 1] = 1000.0 * (1 - 2 * (torch.arange(n) % 2))
    x[T + 2] = torch.tensor([127, .5, 1.5, 2.5, -.5, -1.5, -2.5, 3.5, -0.0, -127, 126.5, -126.5]
                            + [0.0] * 20).repeat(n // 32)
    x = x.to(TDT[dt])
    T, g = T + 3, 32
    want_q, want_s, want_sum = R.quantize(x, g)
    assert want_q.min() == -127 and want_q.max() == 127
    xbuf = torch.full((T, n + pad), 7.0, dtype=x.dtype)
    xbuf[:, :n] = x
    xbuf = xbuf.to(DEV)
    qbuf = torch.full((T, n + pad), 0x5B, dtype=torch.int8, device=DEV)
    sbuf = torch.full((T + 8,), -3.0, dtype=torch.float32, device=DEV)
    ubuf = torch.full((T * (n // g) + 8,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        L.call("tg_quant_act_i8", L.stream(), L.ptr(xbuf), L.DTYPES[x.dtype], T, n + pad, n, g,
               L.ptr(qbuf), n + pad, L.ptr(sbuf[4:]), L.ptr(ubuf[4:]))
    q, s, u = qbuf.cpu().numpy(), sbuf.cpu().numpy(), ubuf.cpu().numpy()
    assert np.all(q[:, n:] == 0x5B) and np.all(s[:4] == -3) and np.all(s[4 + T:] == -3) \
        and np.all(u[:4] == -77) and np.all(u[4 + T * (n // g):] == -77), "padding was written"
    assert np.array_equal(s[4:4 + T].view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(q[:, :n], want_q), f"{np.mean(q[:, :n] != want_q):.4f} of the bytes differ"
    assert np.array_equal(u[4:4 + T * (n // g)].reshape(T, -1), want_sum)


# ---- 2. the GEMM on exact integer data ------------------------------------------------
def run_act(x_view, qw, qz, sc, m, n, g, b, y_view, bias=None):
    L = lib()
    T = x_view.shape[0]
    ldx = x_view.stride(0) if T > 1 else max(x_view.stride(0), n)
    nbytes = L.lib.tg_qgemm_act_workspace_size(T, m, n, g)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm_act", L.stream(), L.ptr(x_view), L.DTYPES[x_view.dtype], T, ldx,
               L.ptr(qw), L.ptr(qz), L.ptr(sc), L.DTYPES[sc.dtype], m, n, g, b, ACT, L.ptr(bias),
               L.DTYPES[bias.dtype] if bias is not None else 0, L.ptr(y_view),
               L.DTYPES[y_view.dtype], y_view.stride(0), L.ptr(ws), nbytes)


def check_exact(b, m, n, g, T, xdt, ydt, bdt):
    """x = q 2^e with q integers in [-3, 3] but one +-127 a row, so xs = 2^e and q
    are exact; scales 2^-6 .. 2^-2 (fp16 and fp32 images alternate); the bias
    multiples of 2^-6.  In units of 2^-7 every term is an integer and their
    absolute sum stays below 2^24: every summation order gives the same bits, and
    the expected image is that exact value rounded once to ydt."""
    codes, zero, scale, qw, qz, sc = R.weights(m, n, g, b, "pow2")
    rng = np.random.default_rng(T + n + b)
    q = rng.integers(-3, 4, size=(T, n))
    q[np.arange(T), rng.integers(0, n, size=T)] = 127 * (1 - 2 * (np.arange(T) % 2))
    e = 2.0 ** (np.arange(T) % 3 - 1)
    bias = (rng.integers(-200, 201, size=m) / 64.0).astype(np.float32) if bdt else None
    y64, mag = R.gemm(q, e.astype(np.float32), codes, zero, scale, g, b, bias)
    assert mag.max() * 128 < 2 ** 24 and np.array_equal(np.rint(y64 * 128), y64 * 128)
    want = torch.from_numpy(y64.astype(np.float32)).to(TDT[ydt])
    pad_x = 8 if T % 2 == 0 else 5                     # 16-byte rows, or scalar loads
    SX, SY = 3.0, -12288.0
    xbuf = torch.full((T, n + pad_x), SX, dtype=TDT[xdt])
    xbuf[:, :n] = torch.from_numpy(q * e[:, None]).to(TDT[xdt])
    xbuf = xbuf.to(DEV)
    ybuf = torch.full((T, m + 5), SY, dtype=TDT[ydt], device=DEV)
    run_act(xbuf[:, :n], dev(qw), dev(qz), dev(sc, TDT["f16" if T % 2 else "f32"]), m, n, g, b,
            ybuf[:, :m], bias=dev(bias, TDT[bdt]) if bdt else None)
    got = ybuf.cpu()
    assert torch.all(got[:, m:] == SY), "the padding of Y was written"
    assert np.array_equal(raw_bits(got[:, :m]), raw_bits(want)), \
        f"{float((got[:, :m] != want).float().mean()):.4f} of the entries differ"


# group inside a step (32), two steps a group (128), one (64), per-channel with a half step
# (160), the 8-bit recentring, the 2- and 3-bit extraction, n below one K step
SHAPES = [(4, 104, 160, 32), (4, 104, 256, 128), (4, 104, 192, 64), (4, 104, 160, -1),
          (8, 104, 160, 32), (2, 96, 128, 64), (3, 96, 160, 32), (4, 104, 32, 32)]
# both sides of the row tiles 16 and 64 and of the switch between them at T = 32
ROWS = (1, 15, 16, 17, 32, 33, 63, 64, 65, 129)
OUT = [(ydt, bdt) for ydt in ("f16", "bf16", "f32") for bdt in (None, "f16", "bf16", "f32")]
EXACT = [s + (T, ("f16", "bf16")[(i + j) % 2]) + OUT[(5 * i + 7 * j) % len(OUT)]
         for i, s in enumerate(SHAPES) for j, T in enumerate(ROWS)]
# the smallest shapes at which the dispatch splits K: 8 steps, two splits of a whole
# number of groups (g = 128: two; g = 32, the two-MFMA step: eight)
EXACT += [(4, 8, 512, 128, 3, "f16", "f16", "f32"), (4, 104, 512, 128, 16, "bf16", "f32", None),
          (4, 104, 512, 32, 5, "f16", "bf16", "bf16"), (8, 104, 512, 128, 40, "bf16", "f32", "f16")]


@pytest.mark.parametrize("b,m,n,g,T,xdt,ydt,bdt", EXACT)
def test_gemm_exact(b, m, n, g, T, xdt, ydt, bdt):
    """m = 104: a full 64-feature tile, then two full 16-tiles and half a one."""
    check_exact(b, m, n, g, T, xdt, ydt, bdt)


# ---- 3. random data against float64 on the quantised operands ---------------------------
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("n,g", [(512, 128), (1024, -1)])
@pytest.mark.parametrize("T", [5, 40])
def test_gemm_numerics_and_determinism(T, n, g, b, xdt, with_bias):
    m = 104
    codes, zero, scale, qw, qz, sc = R.weights(m, n, g, b, "small")
    gen = torch.Generator().manual_seed(T + n)
    x = torch.randn(T, n, generator=gen).to(TDT[xdt])
    bias = (torch.randn(m, generator=gen) * 0.5).to(torch.float16) if with_bias else None
    q, xs, _ = R.quantize(x, g if g > 0 else n)
    y64, mag = R.gemm(q, xs, codes, zero, scale, g, b, bias.float().numpy() if with_bias else None)
    bound = (scale.shape[1] + 4) * 2.0 ** -24 * mag + ulp(y64, xdt)
    x_d, w_d = x.to(DEV), (dev(qw), dev(qz), dev(sc))
    outs = []
    for _ in range(2):
        y = torch.full((T, m), float("nan"), dtype=TDT[xdt], device=DEV)
        run_act(x_d, *w_d, m, n, g, b, y, bias=bias.to(DEV) if with_bias else None)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(raw_bits(outs[0]), raw_bits(outs[1])), "two calls differ"


# ---- 4. module and loader -------------------------------------------------------------------
def test_module_forward_matches_the_abi():
    """A strided 3-D input, x's dtype returned, the bias applied: the ABI call bit
    for bit.  With a rotation and a low-rank pair: the same steps taken by hand."""
    from gptq_svd_amd.qlinear import (QuantLinear, _lowrank_finish, dequantize_act_i8, hadamard,
                                      quantize_act_i8)
    m, n, g, b = 104, 160, 32, 4
    w_d = tuple(dev(t) for t in R.weights(m, n, g, b, "small")[3:])
    gen = torch.Generator().manual_seed(0)
    bias = torch.linspace(-1, 1, m).to(torch.float16).to(DEV)
    x = torch.randn(2, 3, n + 8, generator=gen).half().to(DEV)[..., :n]      # row stride n + 8
    x2 = x.reshape(6, n).contiguous()
    qa = QuantLinear.from_packed(*w_d, b, g, bias=bias, act_format="int8")
    y = qa(x)
    assert y.shape == (2, 3, m) and y.dtype == torch.float16
    y2 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    run_act(x2, *w_d, m, n, g, b, y2, bias=bias)
    assert torch.equal(y.reshape(6, m), y2)
    assert not torch.equal(y, QuantLinear.from_packed(*w_d, b, g, bias=bias)(x))

    xq, xs = quantize_act_i8(x)
    want_q, want_s, _ = R.quantize(x2.cpu(), g)
    assert xq.shape == x.shape and xs.shape == (2, 3) and xq.dtype == torch.int8
    assert np.array_equal(dequantize_act_i8(xq, xs).cpu().numpy().reshape(6, n),
                          want_q.astype(np.float32) * want_s[:, None])

    sign = torch.randint(-2 ** 31, 2 ** 31 - 1, (n // 32,), generator=gen).to(torch.int32).to(DEV)
    lr_a = (torch.randn(m, 4, generator=gen) * 0.1).half().to(DEV)
    lr_b = (torch.randn(4, n, generator=gen) * 0.1).half().to(DEV)
    qr = QuantLinear.from_packed(*w_d, b, g, bias=bias, act_format="int8", lowrank=(lr_a, lr_b),
                                 rotation=(32, sign))
    xr = hadamard(x2, 32, sign)
    y32 = torch.empty(6, m, dtype=torch.float32, device=DEV)
    run_act(xr, *w_d, m, n, g, b, y32)
    y3 = torch.empty(6, m, dtype=torch.float16, device=DEV)
    with torch.cuda.device(DEV):
        _lowrank_finish(xr, 6, n, y32, lr_a, lr_b, bias, y3)
    assert torch.equal(qr(x).reshape(6, m), y3)


def test_loader_installs_the_format(tmp_path):
    from gptq_svd_amd.export import load_quantized, save_quantized
    from gptq_svd_amd.qlinear import QuantLinear

    def model():
        return torch.nn.Sequential(torch.nn.Linear(160, 104, bias=False),
                                   torch.nn.Linear(96, 160, bias=False)).half()

    packed = {name: dict(zip(("qweight", "qzeros", "scales"),
                             (torch.from_numpy(t) for t in R.weights(m, n, 32, 4, "small")[3:])))
              for name, (m, n) in (("0", (104, 160)), ("1", (160, 96)))}
    save_quantized(str(tmp_path), model(), packed, 4, 32, False)
    act = load_quantized(model(), str(tmp_path), device=DEV, act_format="int8")
    plain = load_quantized(model(), str(tmp_path), device=DEV)
    assert [mod.act_format for mod in act if isinstance(mod, QuantLinear)] == ["int8"] * 2
    assert [mod.act_format for mod in plain if isinstance(mod, QuantLinear)] == [None] * 2
    x = torch.randn(5, 160, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    assert torch.isfinite(act[0](x)).all() and not torch.equal(act[0](x), plain[0](x))
    qc = json.load(open(tmp_path / "quantize_config.json"))
    for sub, change, fmt in (("a", {}, "mxfp8"), ("a", {}, "int4"),
                             ("b", dict(checkpoint_format="mxfp4"), "int8"),
                             ("c", dict(experts=["0"]), "int8")):
        (tmp_path / sub).mkdir(exist_ok=True)             # the configuration alone: no tensors
        (tmp_path / sub / "quantize_config.json").write_text(json.dumps(dict(qc, **change)))
        with pytest.raises(ValueError, match="act_format"):
            load_quantized(model(), str(tmp_path / sub), act_format=fmt)
