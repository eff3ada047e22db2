"""GPU: packed inference (A14) at the production dispatch and at its layout
edges -- the paths test_gpu_qlinear.py's small shapes never take.

Cases and host references live in qlinear_ref.py; test_qlinear_ref.py proves on
the CPU that every exact case is exact (so no comparison here is vacuous) and
that the wave-loop shapes reach the wave loop.  All comparisons are bit-exact
except the random-data numerics (i), which uses the bound derived in
test_gpu_qlinear.py.  X, Y and the dequantised weight live inside
sentinel-filled buffers whose whole image is compared: the result, "nothing
outside the logical matrix was written" and "the input was left alone" in one.

  (a) wave loop    m = 4416, n = 2048 (and 2240 x 4096 at 8 bits, 9352 x 2048
                   for three units per wave): the gemv kernel's zero / scale
                   cache, the LDS offset of a wave's later units and the short
                   last K split; the mfma kernel's group carried across slabs
  (b) groups       a boundary inside a slab (96), 64, 256, per-channel
  (c) K tails      n = 32, 64, 160, 224
  (d) features     the smallest legal m per width, one tile plus a step, 128
  (e) row buckets  gemv TT = 2, 4, 8, 16 and the 64- / 128-row mfma tile
  (f) X addressing misaligned base with ldx % 8 == 0, ldx = n + 8, T = 1
  (g) outputs      16-bit Y against one rounding of the exact value (inexact
                   and overflowing values planted), every bias type on the
                   three finishing paths, ldy > m
  (h) auto         T = 4 is the gemv run, T = 5 the mfma run
  (i) numerics     random data at the wave-loop shape, fp16 and fp32 scales
  (j) dequant      short last unit, group switch inside a unit, m > 256,
                   ldo > n, saturating values
  (k) packers      tg_pack_codes / tg_pack_zeros at m > 256 and more than 256
                   zero words per group feed tg_dequant_packed and tg_qgemm
  (l) QuantLinear  a strided 3-D view with a storage offset
"""
import functools

import numpy as np
import pytest
import torch

import qlinear_ref as R
from qlinear_ref import TDT, raw_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def case_id(c):
    return "-".join(str(v) for v in c)


def with_regimes(cases):
    return [pytest.param(c, regime, id=f"{case_id(c)}-{regime}")
            for c in cases for regime in R.regimes(c.T)]


@functools.lru_cache(maxsize=None)
def dev_packed(m, n, g, b, kind, sdt):
    """The packed case on the device (uploaded once per module)."""
    _, _, _, qw, qz, sc = R.packed_case(m, n, g, b, kind)
    return (torch.from_numpy(qw).to(DEV), torch.from_numpy(qz).to(DEV),
            torch.from_numpy(sc).to(TDT[sdt]).to(DEV))


def elem_ptr(t, lead):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + lead * t.element_size())


def qgemm(x_d, x_lead, ldx, T, packed, m, n, g, b, y_d, y_lead, ldy, bias_d=None):
    """tg_qgemm on flat buffers: X at element x_lead of x_d, Y at y_lead of y_d."""
    from gptq_svd_amd import _lib as L
    qw_d, qz_d, sc_d = packed
    nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm", L.stream(), elem_ptr(x_d, x_lead), L.DTYPES[x_d.dtype], T, ldx,
               L.ptr(qw_d), L.ptr(qz_d), L.ptr(sc_d), L.DTYPES[sc_d.dtype], m, n, g, b,
               L.ptr(bias_d), L.DTYPES[bias_d.dtype] if bias_d is not None else 0,
               elem_ptr(y_d, y_lead), L.DTYPES[y_d.dtype], ldy, L.ptr(ws), nbytes)


def same_image(got, want, lead, rows, ld, width, what):
    """Bit equality of two flat images; the message says where they differ."""
    g, w = raw_bits(got), raw_bits(want)
    if np.array_equal(g, w):
        return
    inside = np.zeros(g.shape, dtype=bool)
    inside[lead:lead + rows * ld].reshape(rows, ld)[:, :width] = True
    diff = g != w
    bad = np.argwhere((diff & inside)[lead:lead + rows * ld].reshape(rows, ld))
    first = tuple(bad[0]) if len(bad) else None
    raise AssertionError(
        f"{what}: {np.count_nonzero(diff & inside)} of {rows * width} entries differ (first at "
        f"{first}), {np.count_nonzero(diff & ~inside)} elements outside the matrix were written")


def run_exact(c, regime, monkeypatch, packed=None):
    monkeypatch.setenv("TG_QGEMM", regime)
    ref = R.exact_case(c)
    if packed is None:
        packed = dev_packed(c.m, c.n, c.g, c.b, "pow2", "f16")
    x_img, x_lead, ldx = R.x_image(c, ref["X"])
    x_d = x_img.to(DEV)
    assert x_d.data_ptr() % 16 == 0
    y_img, y_lead, ldy = R.y_image(c.T, c.m, c.ydt)
    y_d = y_img.to(DEV)
    bias_d = None
    if c.bias is not None:
        bias_d = torch.from_numpy(np.array(ref["bias"])).to(TDT[c.bias]).to(DEV)
    qgemm(x_d, x_lead, ldx, c.T, packed, c.m, c.n, c.g, c.b, y_d, y_lead, ldy, bias_d)
    want_img, _, _ = R.y_image(c.T, c.m, c.ydt, ref["want"])
    same_image(y_d.cpu(), want_img, y_lead, c.T, ldy, c.m, "Y")
    same_image(x_d.cpu(), x_img, x_lead, c.T, ldx, c.n, "X (an input)")


# ---- (a) .. (g): exact --------------------------------------------------------
@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_WAVE))
def test_wave_loop_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_GROUP))
def test_group_geometry_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_KTAIL))
def test_k_tails_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_FEAT))
def test_feature_edges_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_ROWS))
def test_row_buckets_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_XADDR))
def test_x_addressing_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


@pytest.mark.parametrize("c,regime", with_regimes(R.CASES_OUT))
def test_outputs_and_bias_exact(c, regime, monkeypatch):
    run_exact(c, regime, monkeypatch)


# ---- (h) auto dispatch --------------------------------------------------------
@pytest.mark.parametrize("xdt", R.XDTS)
def test_auto_dispatch_boundary(xdt, monkeypatch):
    """Random data, fp32 output, n = 1024: the two regimes add in different
    orders, so their bits differ and tell which one ran."""
    m, n, g, b = 96, 1024, 128, 4
    packed = dev_packed(m, n, g, b, "small", "f32")
    x = torch.randn(5, n, generator=torch.Generator().manual_seed(3)).to(TDT[xdt]).to(DEV)

    def run(T, mode):
        if mode is None:
            monkeypatch.delenv("TG_QGEMM", raising=False)
        else:
            monkeypatch.setenv("TG_QGEMM", mode)
        y = torch.full((T, m), float("nan"), dtype=torch.float32, device=DEV)
        qgemm(x, 0, n, T, packed, m, n, g, b, y, 0, m)
        return raw_bits(y)

    gemv4, mfma4, auto4 = run(4, "gemv"), run(4, "mfma"), run(4, None)
    gemv5, mfma5, auto5 = run(5, "gemv"), run(5, "mfma"), run(5, None)
    assert not np.array_equal(gemv4, mfma4) and not np.array_equal(gemv5, mfma5), \
        "the regimes agree bit for bit here: this data cannot tell them apart"
    assert np.array_equal(auto4, gemv4), "T = 4 in auto is not the gemv run"
    assert np.array_equal(auto5, mfma5), "T = 5 in auto is not the mfma run"


# ---- (i) numerics at the wave-loop shape ----------------------------------------
@functools.lru_cache(maxsize=None)
def numerics_case(b, sdt, xdt, T):
    """(x CPU tensor, y64, bound) at the wave-loop shape; the bound is
    test_qgemm_numerics_and_determinism's: 2 n 2^-24 (|X| |W^|^T) + ulp(y64)."""
    m, n, g = R.WAVE_M, R.WAVE_N, 128
    codes, zero, scale, _, _, sc = R.packed_case(m, n, g, b, "small")
    scale_used = torch.from_numpy(sc).to(TDT[sdt]).float().numpy().T   # after the fp16 rounding
    x = torch.randn(T, n, generator=torch.Generator().manual_seed(T + b)).to(TDT[xdt])
    w64 = R.host_dequant(codes, zero, scale_used, g, xdt).double().numpy()
    x64 = x.double().numpy()
    y64 = x64 @ w64.T
    bound = 2 * n * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T) + R.ulp(y64, xdt)
    return x, y64, bound


NUM = [(b, sdt, xdt, T, regime) for b in (3, 4) for sdt in ("f16", "f32")
       for xdt, T in (("f16", 4), ("bf16", 4), ("f16", 16)) for regime in R.regimes(T)]


@pytest.mark.parametrize("b,sdt,xdt,T,regime", NUM)
def test_wave_loop_numerics_and_determinism(b, sdt, xdt, T, regime, monkeypatch):
    m, n, g = R.WAVE_M, R.WAVE_N, 128
    monkeypatch.setenv("TG_QGEMM", regime)
    x, y64, bound = numerics_case(b, sdt, xdt, T)
    packed = dev_packed(m, n, g, b, "small", sdt)
    x_d = x.to(DEV)
    outs = []
    for _ in range(2):
        y = torch.full((T, m), float("nan"), dtype=TDT[xdt], device=DEV)
        qgemm(x_d, 0, n, T, packed, m, n, g, b, y, 0, m)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(raw_bits(outs[0]), raw_bits(outs[1])), "two calls differ"


# ---- (j) dequant through the C ABI ----------------------------------------------
def run_dequant(packed_host, m, n, g, b, sdt, out, qw_d=None, qz_d=None):
    """tg_dequant_packed with ldo = n + 3 into a sentinel-filled buffer; the whole
    image against the host formula."""
    from gptq_svd_amd import _lib as L
    codes, zero, scale, qw, qz, sc = packed_host
    if qw_d is None:
        qw_d, qz_d = torch.from_numpy(qw).to(DEV), torch.from_numpy(qz).to(DEV)
    sc_d = torch.from_numpy(sc).to(TDT[sdt]).to(DEV)
    ldo = n + 3
    img = torch.full((m * ldo + R.TAIL,), R.SENT_Y, dtype=TDT[out])
    out_d = img.to(DEV)
    with torch.cuda.device(DEV):
        L.call("tg_dequant_packed", L.stream(), L.ptr(qw_d), L.ptr(qz_d), L.ptr(sc_d),
               L.DTYPES[sc_d.dtype], m, n, g, b, L.ptr(out_d), L.DTYPES[out_d.dtype], ldo)
    scale_used = sc_d.cpu().float().numpy().T
    want = R.host_dequant(codes, zero, scale_used, g, out)
    img[:m * ldo].view(m, ldo)[:, :n] = want
    same_image(out_d.cpu(), img, 0, m, ldo, n, "dequantised weight")
    return want


@pytest.mark.parametrize("out", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("sdt", ["f16", "f32"])
@pytest.mark.parametrize("shape", R.DEQUANT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_dequant_short_units_odd_groups_many_features(shape, sdt, out):
    m, n, g, b = shape
    run_dequant(R.packed_case(m, n, g, b, "rand"), m, n, g, b, sdt, out)


@pytest.mark.parametrize("out", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("sdt", ["f16", "f32"])
@pytest.mark.parametrize("fill", ["max", "min"])
@pytest.mark.parametrize("shape", R.DEQUANT_FILL_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_dequant_saturating_values(shape, fill, sdt, out):
    m, n, g, b = shape
    want = run_dequant(R.packed_fill(m, n, g, b, fill), m, n, g, b, sdt, out)
    assert bool(torch.isinf(want).all()) == (out == "f16")     # fp16 overflows, the others hold it


# ---- (k) the project's own packers feed the consumers ----------------------------
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("shape", R.PACK_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_packers_feed_dequant_and_qgemm(shape, sym, monkeypatch):
    from gptq_svd_amd import _lib as L
    m, n, g, b = shape
    host = R.packed_case(m, n, g, b, "pow2")
    codes, zero, scale, qw, qz, sc = host
    G = zero.shape[1]
    off = R.oracle().code_offset(b, sym)
    nw, nz = n * b // 32, m * b // 32
    SENT = 0x55555555
    qw_d = torch.full((nw * m + 1,), SENT, dtype=torch.int32, device=DEV)
    qz_d = torch.full((G * nz + 1,), SENT, dtype=torch.int32, device=DEV)
    dc = torch.from_numpy(codes.astype(np.uint8)).to(DEV)                 # stored (unsigned) codes
    dz = torch.from_numpy((zero - off).astype(np.float32)).to(DEV)        # stored zero = zero + off
    with torch.cuda.device(DEV):
        L.call("tg_pack_codes", L.stream(), L.ptr(dc), m, n, b, L.ptr(qw_d))
        L.call("tg_pack_zeros", L.stream(), L.ptr(dz), m, G, b, int(sym), L.ptr(qz_d))
    qw_h, qz_h = qw_d.cpu().numpy(), qz_d.cpu().numpy()
    assert qw_h[-1] == SENT and qz_h[-1] == SENT
    assert np.array_equal(qw_h[:-1].reshape(nw, m), qw), "qweight differs from the oracle's"
    assert np.array_equal(qz_h[:-1].reshape(G, nz), qz), "qzeros differ from the oracle's"
    # the words the GPU packed, through both consumers
    qw_v, qz_v = qw_d[:-1].view(nw, m), qz_d[:-1].view(G, nz)
    run_dequant(host, m, n, g, b, "f32", "f32", qw_d=qw_v, qz_d=qz_v)
    if n % 32 == 0:
        sc_d = torch.from_numpy(sc).to(torch.float16).to(DEV)
        for regime in ("gemv", "mfma"):
            run_exact(R.case(m, n, g, b, 4, "f16"), regime, monkeypatch,
                      packed=(qw_v, qz_v, sc_d))


# ---- (l) QuantLinear.forward on a strided view -------------------------------------
@pytest.mark.parametrize("xdt", R.XDTS)
@pytest.mark.parametrize("lead_shape", [(2, 2), (2, 3)])     # T = 4: gemv in auto; T = 6: mfma
def test_quantlinear_forward_on_a_strided_view(lead_shape, xdt, monkeypatch):
    from gptq_svd_amd.qlinear import QuantLinear
    monkeypatch.delenv("TG_QGEMM", raising=False)
    m, n, g, b = 96, 256, 128, 4
    qw_d, qz_d, sc_d = dev_packed(m, n, g, b, "small", "f16")
    bias = torch.linspace(-1, 1, m).to(TDT[xdt]).to(DEV)
    q = QuantLinear.from_packed(qw_d, qz_d, sc_d, b, g, bias=bias)
    B, S = lead_shape
    wide = n + 8
    store = torch.randn(3 + B * S * wide + 5, generator=torch.Generator().manual_seed(1))
    store = store.to(TDT[xdt]).to(DEV)
    x = store.as_strided((B, S, n), (S * wide, wide, 1), storage_offset=3)
    assert not x.is_contiguous() and x.storage_offset() == 3
    before = store.clone()
    y = q(x)
    y_ref = q(x.contiguous())
    assert y.shape == (B, S, m) and y.dtype == TDT[xdt]
    assert np.array_equal(raw_bits(y), raw_bits(y_ref))
    assert torch.equal(store, before)
    # and the value is the ABI's on the same rows
    y2 = torch.empty(B * S, m, dtype=TDT[xdt], device=DEV)
    qgemm(store, 3, wide, B * S, (qw_d, qz_d, sc_d), m, n, g, b, y2, 0, m, bias)
    assert np.array_equal(raw_bits(y.reshape(B * S, m)), raw_bits(y2))
