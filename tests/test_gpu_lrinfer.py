"""GPU: tg_lr_down, tg_lr_finish and the modules' three-call forward.

  1  exact integer data (tests/lrinfer_ref.py, proved exact on the CPU in
     test_lrinfer_ref.py): Z bit-exact in both regimes, split and unsplit; Y
     the one rounding of the exact value, planted with values that overflow
     fp16 and values that are inexact in the 16-bit types;
  2  every combination of the x, B, A, bias and y types;
  3  layouts: X misaligned and strided (scalar loads), B and A likewise, Z and Y
     with a row stride above their width inside sentinel-filled images;
  4  random data through the whole correction beside a packed GEMM:
     |Y - Y64| <= 2n 2^-24 (|x||W^|^T) + 2(n + r) 2^-24 (|x||B|^T|A|^T) + ulp(y),
     and bit-identical results from call to call;
  5  the modules: forward with the buffers equals the three ABI calls bit for
     bit (on a strided 3-D view too), forward without them equals the single
     call of the entry point it always made.
"""
import itertools

import numpy as np
import pytest
import torch

import lrinfer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = R.TDT


@pytest.fixture(scope="module")
def L():
    from gptq_svd_amd import _lib
    return _lib


def dev(a, dt):
    return R.as_tensor(a, dt).to(DEV)


def same_bits(got, want):
    g, w = R.raw_bits(got), R.raw_bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), \
        f"{np.mean(g != w):.3f} of the entries differ"


def lr_down(L, x, B, r, n, Z=None):
    T = x.shape[0]
    ldx = x.stride(0) if T > 1 else max(x.stride(0), n)
    if Z is None:
        Z = torch.empty((T, r), dtype=torch.float32, device=DEV)
    nbytes = L.lib.tg_lr_down_workspace_size(T, r, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_lr_down", L.stream(), L.ptr(x), L.DTYPES[x.dtype], T, ldx, L.ptr(B),
               L.DTYPES[B.dtype], r, n, B.stride(0), L.ptr(Z), Z.stride(0), L.ptr(ws), nbytes)
    return Z


def lr_finish(L, y32, Z, A, bias, Y):
    T, m = y32.shape
    r = A.shape[1]
    with torch.cuda.device(DEV):
        L.call("tg_lr_finish", L.stream(), L.ptr(y32), y32.stride(0), L.ptr(Z), Z.stride(0),
               L.ptr(A), L.DTYPES[A.dtype], A.stride(0), T, m, r, L.ptr(bias),
               L.DTYPES[bias.dtype] if bias is not None else 0, L.ptr(Y), L.DTYPES[Y.dtype],
               Y.stride(0))
    return Y


# ---------------------------------------------------------------------------
# 1. exact data over the shapes
# ---------------------------------------------------------------------------
DOWN = [(T, n, r, regime) for T in R.TS for n in R.NS for r in R.RS for regime in R.regimes(T)]


@pytest.mark.parametrize("T,n,r,regime", DOWN)
def test_down_exact(L, monkeypatch, T, n, r, regime):
    monkeypatch.setenv("TG_LR_DOWN", regime)
    c = R.exact_case(T, n, r)
    xdt, bdt = R.dtypes_for(T + n + r)[:2]
    Z = lr_down(L, dev(c["X"], xdt), dev(c["B"], bdt), r, n)
    same_bits(Z, R.as_tensor(c["Z"], "f32"))


def test_down_auto_is_one_of_the_regimes(L, monkeypatch):
    """TG_LR_DOWN unset: T <= 16 gives the gemv result, above it the mfma one
    (the data is exact, so this shows only that the dispatch runs)."""
    monkeypatch.delenv("TG_LR_DOWN", raising=False)
    for T in R.TS:
        c = R.exact_case(T, 1024, 33)
        same_bits(lr_down(L, dev(c["X"], "f16"), dev(c["B"], "f16"), 33, 1024),
                  R.as_tensor(c["Z"], "f32"))


FINISH = [(T, r) for T in R.TS for r in R.RS]


@pytest.mark.parametrize("T,r", FINISH)
def test_finish_exact(L, T, r):
    c = R.exact_case(T, 160, r)
    _, _, adt, bias_dt, ydt = R.dtypes_for(T + r)
    bias = dev(c["bias"], bias_dt) if bias_dt else None
    Y = torch.empty((T, R.M), dtype=TDT[ydt], device=DEV)
    lr_finish(L, dev(c["Y32"], "f32"), dev(c["Z"], "f32"), dev(c["A"], adt), bias, Y)
    same_bits(Y, R.rounded(c["y_bias" if bias_dt else "y_nobias"], ydt))


# ---------------------------------------------------------------------------
# 2. every combination of the types
# ---------------------------------------------------------------------------
def test_every_type_combination(L, monkeypatch):
    T, n, r = 5, 160, 8
    c = R.exact_case(T, n, r)
    y32 = dev(c["Y32"], "f32")
    zref = R.as_tensor(c["Z"], "f32")
    count = 0
    for regime in ("gemv", "mfma"):
        monkeypatch.setenv("TG_LR_DOWN", regime)
        for xdt, bdt in itertools.product(("f16", "bf16"), ("f16", "bf16", "f32")):
            Z = lr_down(L, dev(c["X"], xdt), dev(c["B"], bdt), r, n)
            same_bits(Z, zref)
            if regime == "mfma":
                continue
            for adt, bias_dt, ydt in itertools.product(("f16", "bf16", "f32"),
                                                       (None, "f16", "bf16", "f32"),
                                                       ("f16", "bf16", "f32")):
                bias = dev(c["bias"], bias_dt) if bias_dt else None
                Y = torch.empty((T, R.M), dtype=TDT[ydt], device=DEV)
                lr_finish(L, y32, Z, dev(c["A"], adt), bias, Y)
                same_bits(Y, R.rounded(c["y_bias" if bias_dt else "y_nobias"], ydt))
                count += 1
    assert count == 2 * 3 * 3 * 4 * 3


# ---------------------------------------------------------------------------
# 3. layouts
# ---------------------------------------------------------------------------
def image(a, dt, lead, pad, sentinel):
    """`a` inside a sentinel-filled flat allocation: `lead` elements in front,
    row stride = width + pad.  -> (allocation, view)."""
    rows, cols = a.shape
    ld = cols + pad
    flat = torch.full((lead + rows * ld + 7,), sentinel, dtype=TDT[dt], device=DEV)
    view = flat[lead:lead + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(R.as_tensor(a, dt))
    return flat, view


def untouched(flat, view, sentinel):
    """Everything of the allocation outside the view still holds the sentinel."""
    mask = torch.ones_like(flat, dtype=torch.bool)
    lead = (view.data_ptr() - flat.data_ptr()) // flat.element_size()
    rows, cols = view.shape
    idx = lead + (torch.arange(rows, device=DEV)[:, None] * view.stride(0)
                  + torch.arange(cols, device=DEV)[None, :])
    mask[idx.reshape(-1)] = False
    return bool(torch.all(flat[mask] == sentinel))


LAYOUTS = {"odd": (0, 5), "vec": (0, 8), "off1": (1, 8), "off3-odd": (3, 3)}   # (lead, pad)


@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("T,regime", [(4, "gemv"), (4, "mfma"), (40, "mfma")])
@pytest.mark.parametrize("bdt", ["f16", "f32"])
def test_layouts(L, monkeypatch, T, regime, lay, bdt):
    monkeypatch.setenv("TG_LR_DOWN", regime)
    n, r = 520, 33
    lead, pad = LAYOUTS[lay]
    c = R.exact_case(T, n, r)
    xf, x = image(c["X"], "bf16", lead, pad, 3.0)
    bf, B = image(c["B"], bdt, lead, pad, 3.0)
    zf, Z = image(np.zeros((T, r)), "f32", 1, 5, -12288.0)
    lr_down(L, x, B, r, n, Z)
    same_bits(Z, R.as_tensor(c["Z"], "f32"))
    assert untouched(zf, Z, -12288.0)
    af, A = image(c["A"], bdt, lead, pad, 3.0)
    yf32, y32 = image(c["Y32"], "f32", 1, 3, 5.0)
    yf, Y = image(np.zeros((T, R.M)), "f16", 1, 5, -12288.0)
    lr_finish(L, y32, Z, A, None, Y)                                     # null bias
    same_bits(Y, R.rounded(c["y_nobias"], "f16"))
    assert untouched(yf, Y, -12288.0)
    for flat, view, s in ((xf, x, 3.0), (bf, B, 3.0), (af, A, 3.0), (yf32, y32, 5.0)):
        assert untouched(flat, view, s)
    same_bits(x, R.as_tensor(c["X"], "bf16"))


def test_finish_in_place(L):
    """Y may be Y32 itself (fp32 output)."""
    c = R.exact_case(17, 160, 8)
    y = dev(c["Y32"], "f32")
    lr_finish(L, y, dev(c["Z"], "f32"), dev(c["A"], "f16"), dev(c["bias"], "f32"), y)
    same_bits(y, R.rounded(c["y_bias"], "f32"))


# ---------------------------------------------------------------------------
# 4. random data beside a packed GEMM
# ---------------------------------------------------------------------------
def packed_int4(m, n, g=32):
    import qlinear_ref as Q
    codes, zero, scale, qw, qz, sc = Q.packed_case(m, n, g, 4, "small")
    W = {dt: Q.host_dequant(codes, zero, scale, g, dt).double().numpy() for dt in ("f16", "bf16")}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(qweight=t(qw), qzeros=t(qz), scales=t(sc), W=W, g=g)


def packed_mx(m, n, seed=3):
    import mx_ref as MX
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 16, size=(m, n))
    codes[codes == 8] = 0
    byte = rng.integers(119, 123, size=(m, n // 32))
    qw, sc = MX.pack(codes, byte)
    W = MX.decode32(codes, np.repeat(byte, 32, axis=1)).astype(np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(qweight=t(qw), scales=t(sc), W=W)


def qgemm_f32(L, kind, x, p, m, n):
    """The packed GEMM with fp32 output and no bias."""
    T = x.shape[0]
    ldx = x.stride(0) if T > 1 else max(x.stride(0), n)
    y32 = torch.empty((T, m), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        if kind == "int4":
            nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm", L.stream(), L.ptr(x), L.DTYPES[x.dtype], T, ldx,
                   L.ptr(p["qweight"]), L.ptr(p["qzeros"]), L.ptr(p["scales"]),
                   L.DTYPES[p["scales"].dtype], m, n, p["g"], 4, None, 0, L.ptr(y32), L.TG_F32, m,
                   L.ptr(ws), nbytes)
        elif kind == "mx":
            nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm_mx", L.stream(), L.ptr(x), L.DTYPES[x.dtype], T, ldx,
                   L.ptr(p["qweight"]), L.ptr(p["scales"]), L.TG_FMT_MXFP4, m, n, None, 0,
                   L.ptr(y32), L.TG_F32, m, L.ptr(ws), nbytes)
        else:
            nbytes = L.lib.tg_qgemm_mx_act_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm_mx_act", L.stream(), L.ptr(x), L.DTYPES[x.dtype], T, ldx,
                   L.ptr(p["qweight"]), L.ptr(p["scales"]), L.TG_FMT_MXFP4, L.TG_ACT_MXFP8, m, n,
                   None, 0, L.ptr(y32), L.TG_F32, m, L.ptr(ws), nbytes)
    return y32


def three_calls(L, kind, x, p, A, B, bias, ydt):
    T, n = x.shape
    m, r = A.shape
    y32 = qgemm_f32(L, kind, x, p, m, n)
    Z = lr_down(L, x, B, r, n)
    return lr_finish(L, y32, Z, A, bias, torch.empty((T, m), dtype=ydt, device=DEV))


RANDOM = [(T, n, r, xdt, ydt) for T, n, r in [(1, 1024, 8), (5, 160, 33), (17, 1024, 128),
                                              (130, 1024, 64), (40, 32, 1), (4, 520, 8)]
          for xdt, ydt in (("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"))]
WORST = {"ratio": 0.0}


@pytest.mark.parametrize("T,n,r,xdt,ydt", RANDOM)
def test_random_within_the_bound(L, T, n, r, xdt, ydt):
    n32 = n if n % 32 == 0 else n + 32 - n % 32          # the packed GEMM needs n % 32 == 0
    m = R.M
    p = packed_int4(m, n32)
    rng = np.random.default_rng(5000 + T + n + r)
    x = torch.from_numpy(rng.standard_normal((T, n32)).astype(np.float32)).to(TDT[xdt])
    B = torch.from_numpy((rng.standard_normal((r, n32)) * 0.05).astype(np.float32)).to(TDT[xdt])
    A = torch.from_numpy((rng.standard_normal((m, r)) * 0.5).astype(np.float32)).to(torch.float16)
    bias = torch.from_numpy(rng.standard_normal(m).astype(np.float32))
    Y = three_calls(L, "int4", x.to(DEV), p, A.to(DEV), B.to(DEV), bias.to(DEV), TDT[ydt])
    Y2 = three_calls(L, "int4", x.to(DEV), p, A.to(DEV), B.to(DEV), bias.to(DEV), TDT[ydt])
    same_bits(Y, Y2)                                     # bit-identical from call to call
    x64, B64, A64 = x.double().numpy(), B.double().numpy(), A.double().numpy()
    W64 = p["W"][xdt]
    y64 = x64 @ W64.T + (x64 @ B64.T) @ A64.T + bias.double().numpy()
    u = 2.0 ** -24
    bound = (2 * n32 * u * (np.abs(x64) @ np.abs(W64).T)
             + 2 * (n32 + r) * u * ((np.abs(x64) @ np.abs(B64).T) @ np.abs(A64).T)
             + R.ulp(y64, ydt))
    err = np.abs(Y.double().cpu().numpy() - y64)
    ratio = float((err / bound).max())
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"[lrinfer] T={T} n={n32} r={r} {xdt}->{ydt}: worst error / bound {ratio:.3f} "
          f"(so far {WORST['ratio']:.3f})")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------
# 5. the modules
# ---------------------------------------------------------------------------
def lr_factors(m, n, r, dt, seed):
    rng = np.random.default_rng(seed)
    A = torch.from_numpy((rng.standard_normal((m, r)) * 0.5).astype(np.float32)).to(dt)
    B = torch.from_numpy((rng.standard_normal((r, n)) * 0.05).astype(np.float32)).to(dt)
    return A.to(DEV), B.to(DEV)


def make_module(kind, p, lowrank, bias):
    from gptq_svd_amd.qlinear import MXQuantLinear, QuantLinear
    if kind == "int4":
        return QuantLinear.from_packed(p["qweight"], p["qzeros"], p["scales"], 4, p["g"],
                                       bias=bias, lowrank=lowrank)
    return MXQuantLinear.from_packed(p["qweight"], p["scales"], bias=bias, lowrank=lowrank,
                                     act_format="mxfp8" if kind == "mxact" else None)


@pytest.mark.parametrize("kind", ["int4", "mx", "mxact"])
@pytest.mark.parametrize("T", [1, 5, 40])
def test_module_forward_is_the_three_calls(L, kind, T):
    m, n, r = R.M, 160, 8
    p = packed_int4(m, n) if kind == "int4" else packed_mx(m, n)
    A, B = lr_factors(m, n, r, torch.float16, 11)
    bias = torch.linspace(-1, 1, m, dtype=torch.float16, device=DEV)
    mod = make_module(kind, p, (A, B), bias)
    assert set(mod.state_dict()) >= {"lr_a", "lr_b", "qweight", "scales"}
    x = torch.randn((T, n), generator=torch.Generator().manual_seed(T)).to(torch.float16).to(DEV)
    same_bits(mod(x), three_calls(L, kind, x, p, A, B, bias, torch.float16))
    # a strided 3-D view: (2, T, n) cut out of a wider tensor
    wide = torch.randn((2, T, n + 8), generator=torch.Generator().manual_seed(9)).to(
        torch.float16).to(DEV)
    xv = wide[:, :, :n]
    got = mod(xv)
    assert got.shape == (2, T, m)
    want = three_calls(L, kind, xv.reshape(-1, n).contiguous(), p, A, B, bias, torch.float16)
    same_bits(got.reshape(-1, m), want)


@pytest.mark.parametrize("kind", ["int4", "mx", "mxact"])
def test_module_without_buffers_is_the_single_call(L, kind):
    """No lr_a / lr_b: the forward is the one call of the entry point with the
    bias and the 16-bit output, as before this feature."""
    m, n, T = R.M, 160, 5
    p = packed_int4(m, n) if kind == "int4" else packed_mx(m, n)
    bias = torch.linspace(-1, 1, m, dtype=torch.float16, device=DEV)
    mod = make_module(kind, p, None, bias)
    assert mod.lr_a is None and mod.lr_b is None
    assert not {"lr_a", "lr_b"} & set(mod.state_dict())
    x = torch.randn((T, n), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    y = torch.empty((T, m), dtype=torch.bfloat16, device=DEV)
    with torch.cuda.device(DEV):
        if kind == "int4":
            nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm", L.stream(), L.ptr(x), L.TG_BF16, T, n, L.ptr(p["qweight"]),
                   L.ptr(p["qzeros"]), L.ptr(p["scales"]), L.DTYPES[p["scales"].dtype], m, n,
                   p["g"], 4, L.ptr(bias), L.TG_F16, L.ptr(y), L.TG_BF16, m, L.ptr(ws), nbytes)
        elif kind == "mx":
            nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm_mx", L.stream(), L.ptr(x), L.TG_BF16, T, n, L.ptr(p["qweight"]),
                   L.ptr(p["scales"]), L.TG_FMT_MXFP4, m, n, L.ptr(bias), L.TG_F16, L.ptr(y),
                   L.TG_BF16, m, L.ptr(ws), nbytes)
        else:
            nbytes = L.lib.tg_qgemm_mx_act_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)
            L.call("tg_qgemm_mx_act", L.stream(), L.ptr(x), L.TG_BF16, T, n, L.ptr(p["qweight"]),
                   L.ptr(p["scales"]), L.TG_FMT_MXFP4, L.TG_ACT_MXFP8, m, n, L.ptr(bias),
                   L.TG_F16, L.ptr(y), L.TG_BF16, m, L.ptr(ws), nbytes)
    same_bits(mod(x), y)


@pytest.mark.parametrize("kind", ["int4", "mx"])
def test_effective_weight(L, kind):
    """dequantize(effective=True) = W^ + lr_a lr_b as the forward applies it: for
    MXFP4 (whose decoded weights are exact in fp16) an identity input reads it
    back row by row."""
    from gptq_svd_amd.qlinear import add_lowrank
    m, n, r = R.M, 160, 8
    p = packed_int4(m, n) if kind == "int4" else packed_mx(m, n)
    A, B = lr_factors(m, n, r, torch.float16, 12)
    mod = make_module(kind, p, (A, B), None)
    W32 = mod.dequantize(torch.float32)
    eff = mod.dequantize(torch.float32, effective=True)
    same_bits(eff, add_lowrank(W32, A, B))
    want = W32.double() + A.double() @ B.double()
    bound = 2 * r * 2.0 ** -24 * (A.double().abs() @ B.double().abs()) \
        + 2.0 ** -23 * want.abs() + 1e-30
    assert bool(torch.all((eff.double() - want).abs() <= bound))
    same_bits(mod.dequantize(torch.float16), make_module(kind, p, None, None).dequantize())
    if kind == "mx":
        # x = I: y[i, o] = W^[o, i] + sum_j B[j, i] A[o, j], the same fma chain
        eye = torch.eye(n, dtype=torch.float16, device=DEV)
        same_bits(mod(eye).t().contiguous(), eff.to(torch.float16))


def test_from_packed_rejects_bad_factors():
    from gptq_svd_amd.qlinear import QuantLinear
    p = packed_int4(R.M, 160)
    A, B = lr_factors(R.M, 160, 8, torch.float16, 1)
    for bad in ((A[:-1], B), (A, B[:, :-1]), (A[:, :4], B), (A.double(), B.double())):
        with pytest.raises(ValueError):
            QuantLinear.from_packed(p["qweight"], p["qzeros"], p["scales"], 4, p["g"], lowrank=bad)
