"""GPU: grouped packed GEMM with MXFP8 activations (A22), tg_qgemm_grouped_act up
to load_quantized(experts_act_format=...), against the float64 per-expert loop
on the quantised operands (mx_ref.py weights, mxa_ref.py activations).
Shapes: E = 4 with runs [0, 1, 17, 70] (empty, one slot, across a 16-slot tile,
across a 64-slot tile) or all in the last expert; m = 104 (a 40-feature tail);
n = 160 (a one-block K tail, one split) and 1024 (two splits); T = 40 rows of X
feeding several slots each, or rows = None."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import mx_ref as W
import mxa_ref as A
from qlinear_ref import ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
M, E, T = 104, 4, 40
COUNTS = {"mixed": [0, 1, 17, 70], "last": [0, 0, 0, 23]}
VARIANTS = [("f16", True, True, False), ("bf16", False, False, True), ("bf16", True, False, False),
            ("f16", False, True, True)]       # (x dtype, rows given, row_scale given, f32 output)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def splits(L, Tx, R, n):
    """K splits, from the workspace size: Tx n + Tx n/32 bytes, S R M floats (+ 255 each)"""
    rest = int(L.lib.tg_qgemm_grouped_act_workspace_size(Tx, R, E, M, n)) \
        - (Tx * n + 255) - (Tx * (n // 32) + 255)
    assert rest == 0 or (rest - 255) % (R * M * 4) == 0
    return 1 if rest == 0 else (rest - 255) // (R * M * 4)


def grouped_act(L, x, rows, off, qw, sc, n, rs, y, R):
    nbytes = L.lib.tg_qgemm_grouped_act_workspace_size(x.shape[0], R, E, M, n)
    ws = L.workspace(nbytes, DEV)
    with torch.cuda.device(DEV):
        L.call("tg_qgemm_grouped_act", L.stream(), L.ptr(x), L.DTYPES[x.dtype], x.shape[0],
               x.stride(0), L.ptr(rows), L.ptr(off), R, E, L.ptr(qw), L.ptr(sc), 1, 1, M, n,
               L.ptr(rs), L.ptr(y), L.DTYPES[y.dtype], y.stride(0), L.ptr(ws), nbytes)


@functools.lru_cache(maxsize=None)
def case(kind, n, counts, use_rows, xdt="f16"):
    """-> X^ float64, x tensor, W^ (E, M, n) float64, packed pair, offsets, rows, row_scale"""
    rng = np.random.default_rng(n + len(kind))
    off = np.concatenate([[0], np.cumsum(COUNTS[counts])]).astype(np.int32)
    R = int(off[-1])
    rows = rng.integers(0, T, size=R).astype(np.int32) if use_rows else None
    if use_rows:
        rows[1:4] = rows[0]                                 # a token feeds several slots
    Tx = T if use_rows else R
    if kind == "exact":
        cs = [W.exact_gemm_case(M, n, 1, 50 + e, distinct=True) for e in range(E)]
        w64 = np.stack([c["w_int"] for c in cs]).astype(np.float64)
        pk = [W.pack(c["codes"], c["byte"]) for c in cs]
        X = A.exact_x(Tx, n, Tx).astype(np.float64)
        x = torch.from_numpy(X).to(A.TDT[xdt])
        rs = (2.0 ** rng.integers(-1, 2, size=R)).astype(F32)
    else:
        q = [W.rtn((rng.standard_normal((M, n)) * 0.05).astype(F32)) for _ in range(E)]
        w64 = np.stack([W.decode32(c, W.expand(b)) for _, c, _, b in q]).astype(np.float64)
        pk = [W.pack(c, b) for _, c, _, b in q]
        x = torch.randn(Tx, n, generator=torch.Generator().manual_seed(n)).to(A.TDT[xdt])
        X = A.decode(*A.quantize(x)).astype(np.float64)
        rs = (rng.random(R) + 0.1).astype(F32)
    return X, x, w64, (np.stack([p[0] for p in pk]), np.stack([p[1] for p in pk])), off, rows, rs


def reference(X, w64, off, rows, rs):
    """float64 (R, M): the per-expert loop, and the same on the absolute values"""
    idx = np.arange(off[-1]) if rows is None else rows
    y, a = np.zeros((len(idx), M)), np.zeros((len(idx), M))
    for e in range(E):
        s = slice(off[e], off[e + 1])
        y[s] = (X[idx[s]] @ w64[e].T) * rs[s, None]
        a[s] = (np.abs(X[idx[s]]) @ np.abs(w64[e]).T) * np.abs(rs[s, None])
    return y, a


def run(kind, n, counts, xdt, use_rows, use_rs, f32):
    """One call, NaN-filled (R + 2, M + 8) Y, X of row stride n + 8 -> Y, y64, abs64, splits"""
    from gptq_svd_amd import _lib as L
    X, x, w64, (qw, sc), off, rows, rs = case(kind, n, counts, use_rows, xdt)
    R = int(off[-1])
    rs = rs if use_rs else np.ones(R, dtype=F32)
    xbuf = torch.nn.functional.pad(x, (0, 8), value=3.0).to(DEV)
    ybuf = torch.full((R + 2, M + 8), float("nan"), dtype=torch.float32 if f32 else x.dtype,
                      device=DEV)
    grouped_act(L, xbuf[:, :n], dev(rows), dev(off), dev(qw), dev(sc), n,
                dev(rs) if use_rs else None, ybuf[:R, :M], R)
    got = ybuf.cpu()
    assert got[R:].isnan().all() and got[:, M:].isnan().all(), "Y was written outside R x m"
    return (got[:R, :M],) + reference(X, w64, off, rows, rs.astype(np.float64)) \
        + (splits(L, x.shape[0], R, n),)


@pytest.mark.parametrize("xdt,use_rows,use_rs,f32", VARIANTS)
@pytest.mark.parametrize("bm", ["16", "64", "auto"])
@pytest.mark.parametrize("n", [160, 1024])
@pytest.mark.parametrize("counts", list(COUNTS))
def test_exact(counts, n, bm, xdt, use_rows, use_rs, f32, monkeypatch):
    """Exact fp32 sums: the float64 loop bit for bit, both heights, split and unsplit K."""
    monkeypatch.setenv("TG_QGROUPED_ACT", bm)
    got, y64, a64, S = run("exact", n, counts, xdt, use_rows, use_rs, f32)
    assert a64.max() < 2 ** 24, "the reference is not exact"
    assert (S > 1) == (n == 1024), f"{S} splits at n = {n}"
    want = torch.from_numpy(y64.astype(F32)).to(got.dtype)
    assert np.array_equal(W.raw_bits(got), W.raw_bits(want)), "Y differs from the exact result"


@pytest.mark.parametrize("bm", ["64", "auto"])
@pytest.mark.parametrize("xdt", ["f16", "bf16"])
@pytest.mark.parametrize("n", [160, 1024])
def test_numerics_and_determinism(n, xdt, bm, monkeypatch):
    """|y - y64| <= 2 n 2^-24 (|X^| |W^_e|^T) |row_scale| + ulp(y64), test_gpu_mxa.py's bound"""
    monkeypatch.setenv("TG_QGROUPED_ACT", bm)
    outs = [run("random", n, "mixed", xdt, True, True, False) for _ in range(2)]
    got, y64, a64, _ = outs[0]
    bound = 2 * n * 2.0 ** -24 * a64 + ulp(y64, xdt)
    err = np.abs(got.double().numpy() - y64)
    print(f"max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"worst err/bound {np.max(err / bound):.3f}"
    assert np.array_equal(W.raw_bits(got), W.raw_bits(outs[1][0])), "two calls differ"


def test_module_forward():
    """The three steps by hand bit for bit; not the 16-bit module; within twice the
    error of that module fed the dequantised MXFP8 image at both GEMMs."""
    from gptq_svd_amd.qlinear import QuantExperts, dequantize_act_mx, qgemm_grouped, quantize_act_mx
    H, I, K, Tm = 64, 32, 2, 19
    rng = np.random.default_rng(0)
    stacks = []
    for m, n in ((2 * I, H), (H, I)):
        pk = [W.pack(c, b) for _, c, _, b in
              (W.rtn((rng.standard_normal((m, n)) * 0.2).astype(F32)) for _ in range(E))]
        stacks.append(dict(qweight=dev(np.stack([p[0] for p in pk])), qzeros=None,
                           scales=dev(np.stack([p[1] for p in pk]))))
    qa = QuantExperts.from_packed(*stacks, weight_format="mxfp4", act_format="mxfp8")
    qn = QuantExperts.from_packed(*stacks, weight_format="mxfp4")
    assert "act_format=mxfp8" in repr(qa) and "act_format" not in repr(qn)
    assert list(qa.state_dict()) == list(qn.state_dict())
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(Tm, H, generator=gen).bfloat16().to(DEV)
    idx = torch.stack([torch.randperm(E - 1, generator=gen)[:K] for _ in range(Tm)]).to(DEV)
    w = torch.softmax(torch.randn(Tm, K, generator=gen), dim=-1).bfloat16().to(DEV)
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    off = torch.cat([flat.new_zeros(1), torch.bincount(flat, minlength=E).cumsum(0)]).int()

    def recipe(fmt, pre):
        gu = qgemm_grouped(pre(x), (order // K).int(), off, qa.gate_up_qweight, None,
                           qa.gate_up_scales, 4, 32, act_format=fmt)
        h = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        d = qgemm_grouped(pre(h), None, off, qa.down_qweight, None, qa.down_scales, 4, 32,
                          row_scale=w.reshape(-1)[order].float(), act_format=fmt)
        d = d[torch.argsort(order)].view(Tm, K, H).float()
        return (d[:, 0] + d[:, 1]).bfloat16()

    ya, yn = qa(x, idx, w), qn(x, idx, w)
    assert torch.equal(ya, recipe("mxfp8", lambda t: t)) and not torch.equal(ya, yn)
    ye = recipe(None, lambda t: dequantize_act_mx(*quantize_act_mx(t), t.dtype))
    rel_a, rel_e = (float((y.float() - yn.float()).norm() / yn.float().norm()) for y in (ya, ye))
    print(f"|ya - yn| / |yn| = {rel_a:.3e}, emulated {rel_e:.3e}")
    assert rel_a <= 2 * rel_e, (rel_a, rel_e)


def test_loader_and_arguments(tmp_path):
    from gptq_svd_amd import _lib as L
    from gptq_svd_amd.export import load_quantized, save_quantized
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import QuantExperts, qgemm_grouped
    from test_gpu_qexperts import tiny_moe
    model, ids = tiny_moe()
    model = model.to(DEV)
    res = quantize_model(model, ids, pack=True, weight_format="mxfp4", mode="eigh", w_bits=4,
                         group_size=32, eps=1e-2, batch_size=2, device=DEV)
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, False, weight_format="mxfp4")
    fresh = lambda: tiny_moe()[0].half()
    act = load_quantized(fresh(), str(tmp_path), device=DEV, experts_act_format="mxfp8").eval()
    fmts = [mod.act_format for mod in act.modules() if isinstance(mod, QuantExperts)]
    with torch.no_grad():
        assert fmts == ["mxfp8"] * 2 and torch.isfinite(act(torch.cat(ids[:4]).to(DEV)).logits).all()
    with pytest.raises(ValueError, match="act_format"):
        load_quantized(fresh(), str(tmp_path), experts_act_format="int8")
    with pytest.raises(ValueError, match="act_format"):
        load_quantized(fresh(), str(tmp_path), act_format="mxfp8")
    (tmp_path / "int").mkdir()
    (tmp_path / "int" / "quantize_config.json").write_text(json.dumps(dict(
        json.load(open(tmp_path / "quantize_config.json")), checkpoint_format="gptq_v2")))
    with pytest.raises(ValueError, match="mxfp4 checkpoint"):
        load_quantized(fresh(), str(tmp_path / "int"), experts_act_format="mxfp8")
    z = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="MXFP4"):
        qgemm_grouped(torch.zeros(1, 32).half(), None, z, z.view(1, 1, 1), z, z, 4, 32,
                      act_format="mxfp8")
    p = ctypes.c_void_p(256)        # the C entry rejects these before any device work

    def rc(off=p, wfmt=1, act=1, ws_bytes=1 << 20):
        return L.lib.tg_qgemm_grouped_act(None, p, L.TG_F16, T, 128, p, off, 8, E, p, p, wfmt, act,
                                          M, 128, None, p, L.TG_F16, M, p, ws_bytes)
    assert rc(wfmt=0) == -12 and rc(act=2) == -13 and rc(off=None) == -7
    assert rc(ws_bytes=64) == -99 and "workspace" in L.last_error()
