"""tg_qgemm_grouped (A19) through the C ABI: E stacked packed matrices, each on
its own run of slots, against per-expert host products.

Shapes: m = 96 (the second 64-feature tile is partial), n = 32 (one unit) and
160 (a one-unit tail past a 128 slab), E = 5, slot counts [0, 1, 65, 3, 17] (an
empty expert, one row, a 64-slot tile plus one, a short run, a mid run; R = 86,
unaligned offsets), T = 40 with repeated rows.  The rows regime takes the same
pattern cut to its run length: [0, 1, 5, 3, 2].

The exact cases use the integer data of qlinear_ref / mx_ref: X in [-2, 2],
weights that are integers over 64 (over 1 for MXFP4) and a power-of-two
row_scale, so while the sum of absolute terms stays below 2^24 (asserted) every
partial sum of every order is exact in fp32 and Y must match bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mx_ref
from qlinear_ref import TDT, host_dequant, packed_case, raw_bits, ulp, weight_int

DEV = "cuda:0"
gpu = pytest.mark.gpu
M, E, T = 96, 5, 40
COUNTS = {"tiles": [0, 1, 65, 3, 17], "auto": [0, 1, 65, 3, 17], "rows": [0, 1, 5, 3, 2]}
FMTS = {"int2": (2, 32), "int3": (3, 32), "int4g32": (4, 32), "int4pc": (4, -1), "int8": (8, 32),
        "mxfp4": (4, 32)}
SENT = 777.0


@functools.lru_cache(maxsize=None)
def experts(fmt, n, kind):
    """E stacked packed images of one format.  -> (packed numpy arrays (qweight, qzeros or
    None, scales), w: (E, M, n) float64 the decoded weights (kind "pow2": exact integers
    over `den`), den, decode(xdt) -> (E, M, n) float64 of the operand rounded to xdt)."""
    b, g = FMTS[fmt]
    if fmt == "mxfp4":
        rng = np.random.default_rng(n)
        cs = [mx_ref.exact_gemm_case(M, n, 1, 50 + e, distinct=True) for e in range(E)]
        if kind != "pow2":      # every code, scales 2^-6 .. 2^-3
            for c in cs:
                c["codes"] = rng.integers(0, 16, size=(M, n)).astype(np.uint8)
                c["byte"] = rng.integers(121, 125, size=(M, n // 32)).astype(np.uint8)
        pk = [mx_ref.pack(c["codes"], c["byte"]) for c in cs]
        packed = (np.stack([p[0] for p in pk]), None, np.stack([p[1] for p in pk]))
        dec = lambda xdt: np.stack([mx_ref.decode(c["codes"], mx_ref.expand(c["byte"]), xdt)
                                    .double().numpy() for c in cs])
        return packed, dec("f32"), 1, dec
    cs = [packed_case(M, n, g, b, kind, seed=e) for e in range(E)]
    packed = tuple(np.stack([c[i] for c in cs]) for i in (3, 4, 5))
    dec = lambda xdt: np.stack([host_dequant(c[0], c[1], c[2], g, xdt).double().numpy()
                                for c in cs])
    if kind == "pow2":
        return packed, np.stack([weight_int(c[0], c[1], c[2], g) for c in cs]) / 64.0, 64, dec
    return packed, dec("f32"), 1, dec


def routing(counts, seed=0):
    """(offsets int32 (E + 1), rows int32 (R) with repeats, row_scale f32 powers of two)"""
    rng = np.random.default_rng(seed)
    R = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = rng.integers(0, T, size=R).astype(np.int32)
    rows[1:4] = rows[0]                                   # a row feeds several slots
    return off, rows, (2.0 ** rng.integers(-1, 2, size=R)).astype(np.float32)


def grouped(x, rows, off, packed, fmt, n, rs, y, R=None, ws_bytes=None):
    """The C ABI directly; tensors on the device (rows / rs may be None)."""
    from gptq_svd_amd import _lib as L
    b, g = FMTS[fmt]
    qw, qz, sc = packed
    R = (rows.numel() if rows is not None else x.shape[0]) if R is None else R
    nbytes = L.lib.tg_qgemm_grouped_workspace_size(R, E, M, n) if ws_bytes is None else ws_bytes
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm_grouped", L.stream(), L.ptr(x), L.DTYPES[x.dtype], x.shape[0],
               x.stride(0), L.ptr(rows), L.ptr(off), R, E, L.ptr(qw), L.ptr(qz), L.ptr(sc),
               L.DTYPES[sc.dtype] if qz is not None else 0, int(fmt == "mxfp4"), M, n, g, b,
               L.ptr(rs), L.ptr(y), L.DTYPES[y.dtype], y.stride(0), L.ptr(ws), nbytes)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_packed(packed, sdt=torch.float16):
    qw, qz, sc = (dev(a) for a in packed)
    return qw, qz, sc if sc.dtype == torch.uint8 else sc.to(sdt)


def reference(X64, W64, off, rows, rs):
    """float64 (R, M): the per-expert products times row_scale, and the sums of the
    absolute terms before row_scale"""
    y = np.zeros((len(rows), M))
    a = np.zeros((len(rows), M))
    for e in range(E):
        s = slice(off[e], off[e + 1])
        y[s] = (X64[rows[s]] @ W64[e].T) * rs[s, None]
        a[s] = np.abs(X64[rows[s]]) @ np.abs(W64[e]).T
    return y, a


@gpu
@pytest.mark.parametrize("regime", ["tiles", "auto", "rows"])
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("n", [32, 160])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_grouped_exact(fmt, n, xdt, regime, monkeypatch):
    monkeypatch.setenv("TG_QGROUPED", regime)
    packed, W, den, _ = experts(fmt, n, "pow2")
    off, rows, rs = routing(COUNTS[regime])
    R = len(rows)
    X = np.random.default_rng(n).integers(-2, 3, size=(T, n))
    y64, a64 = reference(X.astype(np.float64), W, off, rows, rs.astype(np.float64))
    assert a64.max() * den < 2 ** 24, "the reference is not exact"
    x = torch.full((T, n + 8), 3.0, dtype=TDT[xdt])
    x[:, :n] = torch.from_numpy(X).to(TDT[xdt])
    x = x.to(DEV)[:, :n]
    y = torch.full((R, M + 8), SENT, dtype=torch.float32, device=DEV)
    grouped(x, dev(rows), dev(off), dev_packed(packed), fmt, n, dev(rs), y[:, :M])
    got = y.cpu().numpy()
    assert np.all(got[:, M:] == SENT), "padding of Y was written"
    want = y64.astype(np.float32)
    assert np.array_equal(got[:, :M], want), f"{np.mean(got[:, :M] != want):.3f} differ"


@gpu
@pytest.mark.parametrize("regime", ["tiles", "rows"])
def test_null_rows_is_the_identity_map(regime, monkeypatch):
    monkeypatch.setenv("TG_QGROUPED", regime)
    n, fmt = 160, "int4g32"
    off = routing(COUNTS[regime])[0]
    R = int(off[-1])
    x = torch.randn(R, n, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    p = dev_packed(experts(fmt, n, "small")[0])
    ys = [torch.zeros(R, M, dtype=torch.float16, device=DEV) for _ in range(2)]
    grouped(x, None, dev(off), p, fmt, n, None, ys[0])
    grouped(x, dev(np.arange(R, dtype=np.int32)), dev(off), p, fmt, n, None, ys[1])
    assert ys[0].abs().max() > 0 and torch.equal(ys[0], ys[1])


@gpu
@pytest.mark.parametrize("regime", ["tiles", "rows"])
@pytest.mark.parametrize("fmt,xdt", [("int4g32", "f16"), ("mxfp4", "bf16")])
def test_grouped_numerics_and_determinism(fmt, xdt, regime, monkeypatch):
    monkeypatch.setenv("TG_QGROUPED", regime)
    n = 160
    packed, _, _, dec = experts(fmt, n, "small")
    off, rows, _ = routing(COUNTS[regime], seed=3)
    R = len(rows)
    gen = torch.Generator().manual_seed(R)
    x = torch.randn(T, n, generator=gen).to(TDT[xdt])
    rs = torch.rand(R, generator=gen) + 0.1
    # fp32 scales: the decoded operand is host_dequant's of the unrounded scale
    y64, a64 = reference(x.double().numpy(), dec(xdt), off, rows, rs.double().numpy())
    bound = 2 * n * 2.0 ** -24 * a64 * rs.double().numpy()[:, None] + ulp(y64, xdt)
    p = dev_packed(packed, torch.float32)
    outs = []
    for _ in range(2):
        y = torch.full((R, M), float("nan"), dtype=TDT[xdt], device=DEV)
        grouped(x.to(DEV), dev(rows), dev(off), p, fmt, n, rs.to(DEV), y)
        outs.append(y.cpu())
    err = np.abs(outs[0].double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(raw_bits(outs[0]), raw_bits(outs[1])), "two calls differ"


@gpu
@pytest.mark.parametrize("regime", ["tiles", "rows"])
def test_empty_call_and_all_slots_in_the_last_expert(regime, monkeypatch):
    monkeypatch.setenv("TG_QGROUPED", regime)
    n, fmt, R = 32, "int8", 7
    packed, W, _, _ = experts(fmt, n, "pow2")
    p = dev_packed(packed)
    X = np.random.default_rng(2).integers(-2, 3, size=(T, n))
    x = torch.from_numpy(X).half().to(DEV)
    off = np.array([0] * E + [R], dtype=np.int32)
    rows = np.arange(R, dtype=np.int32) * 3
    y = torch.full((R, M), SENT, dtype=torch.float32, device=DEV)
    grouped(x, dev(rows), dev(off), p, fmt, n, None, y, R=0)
    assert bool((y == SENT).all()), "R = 0 wrote Y"
    grouped(x, dev(rows), dev(off), p, fmt, n, None, y)
    assert np.array_equal(y.cpu().numpy(), (X[rows] @ W[E - 1].T).astype(np.float32))


def test_argument_errors_without_device_work(monkeypatch):
    """Rejected with the argument's index before anything touches the device
    (fake non-null pointers; runs without a GPU)."""
    from gptq_svd_amd import _lib as L
    p = ctypes.c_void_p(256)

    def rc(R=8, Ex=E, n=128, wfmt=0, bits=4, group=32, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.lib.tg_qgemm_grouped_workspace_size(R, Ex, M, n)
        return L.lib.tg_qgemm_grouped(None, p, L.TG_F16, T, n, p, p, R, Ex, p, p, p, L.TG_F16, wfmt,
                                      M, n, group, bits, None, p, L.TG_F16, M, p, ws_bytes)

    monkeypatch.delenv("TG_QGROUPED", raising=False)
    assert rc(Ex=0) == -9 and rc(Ex=257) == -9
    assert rc(n=48) == -16
    assert rc(wfmt=2) == -14
    assert rc(wfmt=1, bits=3) == -18
    assert rc(ws_bytes=64) == -99 and "workspace" in L.last_error()
    monkeypatch.setenv("TG_QGROUPED", "rows")
    assert rc(R=129, ws_bytes=0) == -8 and "argument 8" in L.last_error()
